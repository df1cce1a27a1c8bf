#!/usr/bin/env python3
"""Loss fixtures: the imported reference (CPU, fp32, eval mode) runs ``GaussianDiffusion.training_losses`` (models/gaussian_diffusion.py:1319-1426)
on the full 1000-step process, B = 3, one window of ``n_poses`` frames, per-row timesteps (0, 500, 999).  Reuses make_golden.py's helpers; same
rules (inputs are seeds, only outputs are stored): weights ``make_synthetic_state_dict(1234)``, conditioning ``make_inputs(seed 5)``, x0 ~ N(0, 1)
from ``torch.Generator().manual_seed(43)``, noise ``SeededNoise(107).randn((B, T, C))`` passed as ``noise=``.

The numbers of ``backward_G`` (trainers/ddpm_beat_trainer.py:222-260; the SHOW trainer's are the same code) are computed here with its formulas
written out — the trainer is not imported — twice: in torch fp32 on the returned dict, as the trainer would, and in float64 from the model output
``pred``, the noise, x0 and the reference's own x_t.  The float64 values are what is stored (a float64 replay of the formulas reproduces them to
round-off of the sums); the fp32 values must agree with them to fp32 accuracy, which ties the stored numbers to the reference's run.  Two quirks of
backward_G are part of the expected values: line 231 recomputes ``loss_model_pred`` over all channels (``expr_weight`` has no effect), and line 247
adds the unscaled ``loss_vel_rec`` to ``final_loss``.

  losses_show.npz      SHOW weights, classifier-free guidance at the config's cond_scale 1.25 (the guided eps is scored)
  losses_show_cs1.npz  SHOW weights, opt.cond_scale = 1: the conditional model
  losses_beat.npz      BEAT weights (no classifier-free guidance)
each: t [B], the seeds, ``pred`` (the model output, so that the formulas can be replayed without the model), ``mse`` [B], ``frame_mse`` [B, T]
(``mse_criterion(...).mean(-1)``), ``loss_model_pred`` / ``loss_vel_rec`` / ``loss_x0_rec`` / ``final_loss``, all float64.

Usage:  python tests/golden/make_golden_losses.py [--only show,show_cs1,beat] [--out DIR]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from make_golden import SeededNoise, build_ref_model, build_ref_samplers, get_config, make_inputs, ref_opt  # noqa: E402

B, X0_SEED, INPUT_SEED, NOISE_SEED = 3, 43, 5, 107
T_ROWS = (0, 500, 999)
HUBER_BETA = float(np.float32(0.1))                # trainers/loss_factory.py:20: 0.1, applied to fp32 tensors
FP32_AGREES = 1e-4                                 # fp32 sums of ~6e4 terms, cancellation at c1 = 158 included
CASES = {"show": ("show", None), "show_cs1": ("show", 1.0), "beat": ("beat", None)}


def backward_g_numbers(out, T: int):
    """ddpm_beat_trainer.py:222-260 on the dict of training_losses, cur_len = T for every row (forward(), :151)."""
    fake_noise, real_noise = out["pred"], out["target"]
    src_mask = torch.ones(fake_noise.shape[0], T)
    frame_mse = ((fake_noise - real_noise) ** 2).mean(dim=-1)                                   # :231 (overwrites :223-230)
    loss_model_pred = 1000 * ((frame_mse * src_mask).sum() / src_mask.sum())                   # :232-233
    vel = ((out["pred_vel"] - out["target_vel"]) ** 2).mean(dim=-1)                             # :242
    vel = (vel * src_mask[:, :-1]).sum() / src_mask[:, :-1].sum()                               # :243
    loss_vel_rec = 100 * vel                                                                    # :245
    huber = torch.nn.functional.smooth_l1_loss(out["target_x0"] / HUBER_BETA, out["pred_x0"] / HUBER_BETA, reduction="mean") * HUBER_BETA
    loss_x0_rec = 100 * huber                                                                   # :253-255
    final_loss = loss_model_pred + vel + loss_x0_rec                                            # :234, :247 (unscaled), :257
    return frame_mse, loss_model_pred, loss_vel_rec, loss_x0_rec, final_loss


def formulas_f64(pred, noise, x_t, x0, c1, c2):
    """The same lines in float64 from the fp32 tensors (c1 / c2 [B]: the fp32 coefficients the reference extracts)."""
    e, nz, xt, x = (v.double() for v in (pred, noise, x_t, x0))
    xp = c1.double().view(-1, 1, 1) * xt - c2.double().view(-1, 1, 1) * e
    frame_mse = ((e - nz) ** 2).mean(dim=-1)
    vel = (((xp[:, :-1] - xp[:, 1:]) - (x[:, :-1] - x[:, 1:])) ** 2).mean(dim=-1)
    vel = vel.sum() / vel.numel()
    z = (x / HUBER_BETA - xp / HUBER_BETA).abs()
    huber = torch.where(z < 1, 0.5 * z * z, z - 0.5).mean() * HUBER_BETA
    lmp, lx0 = 1000 * frame_mse.mean(), 100 * huber
    return frame_mse, frame_mse.mean(dim=-1), lmp, 100 * vel, lx0, lmp + vel + lx0


def gen(tr, gd, rs, tag: str, out_dir: str):
    ds, cond_scale = CASES[tag]
    cfg = get_config(ds) if cond_scale is None else get_config(ds, cond_scale=cond_scale)
    opt = ref_opt(cfg)
    model, _ = build_ref_model(tr, cfg, opt)
    full, _ = build_ref_samplers(gd, rs, opt)
    T, C = cfg.n_poses, cfg.net_dim_pose
    inp = make_inputs(cfg, B, seed=INPUT_SEED)
    x0 = torch.randn(B, T, C, generator=torch.Generator().manual_seed(X0_SEED))
    noise = SeededNoise(NOISE_SEED).randn((B, T, C))
    t = torch.tensor(T_ROWS, dtype=torch.long)
    kw = {"audio_emb": inp["audio_emb"], "length": torch.full((B,), T), "person_id": inp["person_id"],
          "add_cond": {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "y": {}, "pe_type": "pe_sinu"}
    t0 = time.time()
    with torch.no_grad():
        out = full.training_losses(model, x0, t, model_kwargs=kw, noise=noise)
        ref32 = backward_g_numbers(out, T)
        x_t = full.q_sample(x0, t, noise=noise)
    assert torch.equal(out["target"], noise) and out["target_x0"] is x0
    c1 = torch.from_numpy(full.sqrt_recip_alphas_cumprod)[t].float()
    c2 = torch.from_numpy(full.sqrt_recipm1_alphas_cumprod)[t].float()
    frame_mse, mse, lmp, lvr, lx0, final = formulas_f64(out["pred"], noise, x_t, x0, c1, c2)
    for name, a, b in zip(("frame_mse", "loss_model_pred", "loss_vel_rec", "loss_x0_rec", "final_loss", "mse"), ref32 + (out["mse"],),
                          (frame_mse, lmp, lvr, lx0, final, mse)):
        rel = float(((a.double() - b).abs() / b.abs()).max())
        assert rel < FP32_AGREES, (name, rel)
    print(f"  {tag}: {time.time() - t0:.1f}s, mse {mse.tolist()}, loss_model_pred {float(lmp):.6g}, loss_vel_rec {float(lvr):.6g}, "
          f"loss_x0_rec {float(lx0):.6g}, final_loss {float(final):.6g}")
    path = os.path.join(out_dir, f"losses_{tag}.npz")
    np.savez_compressed(path, dataset=ds, batch=B, frames=T, input_seed=INPUT_SEED, x0_seed=X0_SEED, noise_seed=NOISE_SEED, t=t.numpy(),
                        cond_scale=float(opt.cond_scale), huber_beta=HUBER_BETA, pred=out["pred"].numpy(), mse=mse.numpy(),
                        frame_mse=frame_mse.numpy(), loss_model_pred=float(lmp), loss_vel_rec=float(lvr), loss_x0_rec=float(lx0),
                        final_loss=float(final))
    print(f"  wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    torch.set_num_threads(8)
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(CASES))
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    tr, gd, rs, _ = mg.import_reference(with_trainer=False)
    for tag in args.only.split(","):
        gen(tr, gd, rs, tag, args.out)


if __name__ == "__main__":
    main()
