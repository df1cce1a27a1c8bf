"""Float64 reference of the denoising loss terms (dsh_op_denoise_losses, include/diffsheg_hip.h) and of the batch scalars in the formulas of the
reference's backward_G (trainers/ddpm_beat_trainer.py:222-260), numpy only.  Also the SAME formulas evaluated by torch in float32 on the CPU, as
the reference itself would compute them: its error against the float64 values is the yardstick of the op tests' gates."""
from __future__ import annotations

import numpy as np
import torch

LOSS_COLS = 7
SCALARS = ("loss_model_pred", "loss_vel_rec", "loss_x0_rec", "final_loss")
HUBER_BETA = float(np.float32(0.1))       # trainers/loss_factory.py:19-27: beta = 0.1, applied to fp32 tensors


def _np64(a):
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)


def _smooth_l1(a, b):
    z = np.abs(a - b)
    return np.where(z < 1.0, 0.5 * z * z, z - 0.5)


def row_terms_f64(eps, noise, x_t, x0, c1, c2, split: int, beta: float = HUBER_BETA, lens=None) -> np.ndarray:
    """[B, 7]: sum (eps - noise)^2 over the gesture | expression columns, sum (x0_pred - x0)^2, sum over frame pairs of
    ((x0_pred[f] - x0_pred[f+1]) - (x0[f] - x0[f+1]))^2, sum smooth_l1(x0 / beta, x0_pred / beta), element count, pair count — every row
    over its own first lens[b] frames only."""
    eps, noise, x_t, x0 = (_np64(v) for v in (eps, noise, x_t, x0))
    c1, c2 = _np64(c1).reshape(-1), _np64(c2).reshape(-1)
    B, T, C = eps.shape
    out = np.zeros((B, LOSS_COLS))
    for b in range(B):
        n = T if lens is None else int(lens[b])
        e, nz, xt, x = eps[b, :n], noise[b, :n], x_t[b, :n], x0[b, :n]
        xp = c1[b] * xt - c2[b] * e
        d = (e - nz) ** 2
        dv = (xp[:-1] - xp[1:]) - (x[:-1] - x[1:])
        out[b] = [d[:, :split].sum(), d[:, split:].sum(), ((xp - x) ** 2).sum(), (dv ** 2).sum(), _smooth_l1(x / beta, xp / beta).sum(),
                  n * C, max(n - 1, 0)]
    return out


def frame_mse_f64(eps, noise, lens=None) -> np.ndarray:
    """[B, T]: mean over C of (eps - noise)^2, 0 behind a row's length (mse_criterion(...).mean(-1) times src_mask)."""
    eps, noise = _np64(eps), _np64(noise)
    m = ((eps - noise) ** 2).mean(-1)
    if lens is not None:
        for b, n in enumerate(lens):
            m[b, int(n):] = 0.0
    return m


def scalars_f64(rows: np.ndarray, C: int, beta: float = HUBER_BETA) -> dict:
    """backward_G's numbers from the row terms.  Mirrored literally: loss_model_pred is over all channels (line 231 overwrites the
    expr_weight form), and final_loss adds the UNSCALED velocity term (line 247 adds the local loss_vel_rec, not self.loss_vel_rec)."""
    rows = np.asarray(rows, dtype=np.float64)
    frames = (rows[:, 5] / C).sum()
    pairs = rows[:, 6].sum()
    model_pred = (rows[:, 0] + rows[:, 1]).sum() / C / frames
    vel = rows[:, 3].sum() / C / pairs if pairs > 0 else float("nan")
    hub = rows[:, 4].sum() / rows[:, 5].sum() * beta
    out = {"loss_model_pred": 1000.0 * model_pred, "loss_vel_rec": 100.0 * vel, "loss_x0_rec": 100.0 * hub}
    out["final_loss"] = out["loss_model_pred"] + vel + out["loss_x0_rec"]
    return out


def row_terms_f32(eps, noise, x_t, x0, c1, c2, split: int, beta: float = HUBER_BETA, lens=None) -> np.ndarray:
    """The row terms as torch computes them in float32 on the CPU (products, differences, squares and sums all fp32)."""
    eps, noise, x_t, x0 = (torch.as_tensor(v, dtype=torch.float32).cpu() for v in (eps, noise, x_t, x0))
    c1, c2 = torch.as_tensor(c1, dtype=torch.float32).reshape(-1), torch.as_tensor(c2, dtype=torch.float32).reshape(-1)
    B, T, C = eps.shape
    out = np.zeros((B, LOSS_COLS))
    for b in range(B):
        n = T if lens is None else int(lens[b])
        e, nz, xt, x = eps[b, :n], noise[b, :n], x_t[b, :n], x0[b, :n]
        xp = c1[b] * xt - c2[b] * e
        d = (e - nz) ** 2
        dv = (xp[:-1] - xp[1:]) - (x[:-1] - x[1:])
        hub = torch.nn.functional.smooth_l1_loss(x / beta, xp / beta, reduction="sum")
        out[b] = [float(d[:, :split].sum()), float(d[:, split:].sum()), float(((xp - x) ** 2).sum()), float((dv ** 2).sum()), float(hub),
                  n * C, max(n - 1, 0)]
    return out
