"""Restatement of the guided sampler steps for the tests: the guidance energy's gradient and the guided DDIM /
DPM-Solver++(2M) / DDPM updates, written once over plain operators so that the same text runs on numpy float64 arrays (the reference of
the op-level and loop-replay tests) and on fp32 torch CPU tensors (the yardstick of their gates: 4 x the error of that run).

Also the seeded guidance terms of the reference fixtures (tests/golden/make_golden_motion_guidance.py and tests/test_gpu_motion_guidance.py
build the very same tensors from them)."""
from __future__ import annotations

import numpy as np
import torch


# ---- array shims: numpy arrays and torch tensors through one text ----------------------------------------------------------------
def _is_t(a):
    return isinstance(a, torch.Tensor)


def _where(c, a, b):
    return torch.where(c, a, b) if _is_t(a) else np.where(c, a, b)


def _cat(parts, axis):
    return torch.cat(parts, axis) if _is_t(parts[0]) else np.concatenate(parts, axis)


def _clip(a):
    return a.clamp(-1.0, 1.0) if _is_t(a) else np.clip(a, -1.0, 1.0)


def _zeros(a):
    return torch.zeros_like(a) if _is_t(a) else np.zeros_like(a)


def _idx(like, B, T, lengths):
    """frame index [1, T, 1] and lengths [B, 1, 1] (bool-mask material), in like's array family"""
    t = np.arange(T).reshape(1, T, 1)
    L = np.full((B, 1, 1), T) if lengths is None else np.asarray(lengths, dtype=np.int64).reshape(B, 1, 1)
    return (torch.from_numpy(t), torch.from_numpy(L)) if _is_t(like) else (t, L)


def _scalar(like, v):
    """v in like's dtype (an fp32 run rounds its scalars to fp32, like the kernel's arguments)"""
    return torch.tensor(v, dtype=like.dtype) if _is_t(like) else like.dtype.type(v)


def _shift(u, k):
    """u[:, t + k], zeros outside"""
    if k == 0:
        return u
    T = u.shape[1]
    fill = _zeros(u[:, :min(abs(k), T)])
    return _cat([u[:, k:], fill], 1) if k > 0 else _cat([fill, u[:, :k]], 1)


def grad(z, Y, W, lv, la, lengths, scale):
    """g = scale * d log p / d z; z [B, T, C]; Y / W [B, T, C] or None; lv / la [C] or None; lengths: list or None"""
    B, T, C = z.shape
    t, L = _idx(z, B, T, lengths)
    zero = _zeros(z)
    total = _zeros(z)
    if W is not None:
        total = W * (z - (Y if Y is not None else zero))
    if lv is not None:
        v = _where(t <= L - 2, _shift(z, 1) - z, zero)
        total = total + lv.reshape(1, 1, C) * (_shift(v, -1) - v)
    if la is not None:
        a = _where((t >= 1) & (t <= L - 2), (_shift(z, 1) - 2 * z) + _shift(z, -1), zero)
        total = total + la.reshape(1, 1, C) * ((_shift(a, -1) - 2 * a) + _shift(a, 1))
    return _where(t < L, -(_scalar(z, scale) * total), zero)


def _select(x, new, lengths, cols):
    """new inside the clips' frames and the column range, x elsewhere"""
    B, T, C = x.shape
    t, L = _idx(x, B, T, lengths)
    c = np.arange(C).reshape(1, 1, C)
    c = torch.from_numpy(c) if _is_t(x) else c
    lo, hi = cols if cols and cols[1] > cols[0] else (0, C)
    return _where((t < L) & (c >= lo) & (c < hi), new, x)


def _fade(like, L):
    """torch.linspace(0, 1, L) in like's array family and dtype (fp32: torch's own values, which the kernel reproduces)"""
    if _is_t(like):
        return torch.linspace(0, 1, L, dtype=like.dtype)
    return np.linspace(0.0, 1.0, L).astype(like.dtype)


def repaint(new, rp, s):
    """The RePaint select behind a DDIM step (gaussian_diffusion.py:1034-1056): rp = dict(mask bool, gt, noise2, L, blend, tail_blend);
    s: the step's scalars (sqrt_ab_prev, sqrt_1m_ab_prev)."""
    g = s["sqrt_ab_prev"] * rp["gt"] + s["sqrt_1m_ab_prev"] * rp["noise2"]
    L, T = rp["L"], new.shape[1]
    if rp["blend"] and L > 0:
        w = _fade(new, L).reshape(1, L, 1)
        head = g[:, :L] * (1 - w) + new[:, :L] * w
        if rp.get("tail_blend"):
            wt = _fade(new, L).flip(0).reshape(1, L, 1) if _is_t(new) else _fade(new, L)[::-1].reshape(1, L, 1)
            tail = g[:, T - L:] * (1 - wt) + new[:, T - L:] * wt
            g = _cat([head, g[:, L:T - L], tail], 1)
        else:
            g = _cat([head, g[:, L:]], 1)
    return _where(rp["mask"], g, new)


def guided_ddim(x, eps, guide, sc, space, clip=False, lengths=None, cols=None, noise1=None, hist=None, second=False, rp=None):
    """One guided DDIM (or second-order DPM2M) step.  guide: dict(Y, W, lv, la, scale); sc: dict of the step's scalars (c1, c2,
    sqrt_ab_prev, coef_eps, sigma, sqrt_1m_ab, A, Bc, G; with rp also sqrt_1m_ab_prev); rp: the RePaint select behind the update
    (repaint()).  Returns (x_new, x0_guided); elements outside the clips / the columns keep x (and hist)."""
    s = {k: _scalar(x, v) for k, v in sc.items()}
    c1x = s["c1"] * x
    x0 = c1x - s["c2"] * eps
    if clip:
        x0 = _clip(x0)
    z = x if space == "x_t" else x0
    g = grad(z, guide.get("Y"), guide.get("W"), guide.get("lv"), guide.get("la"), lengths, guide.get("scale", 1.0))
    e = (c1x - x0) / s["c2"] - s["sqrt_1m_ab"] * g
    x0g = _where(g == 0, x0, c1x - s["c2"] * e)
    if second:
        D = x0g + s["G"] * (x0g - hist)
        new = s["A"] * x + s["Bc"] * D
    else:
        e2 = (c1x - x0g) / s["c2"]
        new = x0g * s["sqrt_ab_prev"] + s["coef_eps"] * e2
        if noise1 is not None:
            new = new + s["sigma"] * noise1
    if rp is not None:
        new = repaint(new, rp, s)
    return _select(x, new, lengths, cols), (_select(hist, x0g, lengths, cols) if hist is not None else x0g)


def guided_ddpm(x, eps, noise, guide, sc, space, clip=False, lengths=None, cols=None):
    """One guided DDPM step; sc: c1, c2, coef1, coef2, sigma, post_var."""
    s = {k: _scalar(x, v) for k, v in sc.items()}
    x0 = s["c1"] * x - s["c2"] * eps
    if clip:
        x0 = _clip(x0)
    z = x if space == "x_t" else x0
    g = grad(z, guide.get("Y"), guide.get("W"), guide.get("lv"), guide.get("la"), lengths, guide.get("scale", 1.0))
    mean = s["coef1"] * x0 + s["coef2"] * x
    mean = _where(g == 0, mean, mean + s["post_var"] * g)
    return _select(x, mean + s["sigma"] * noise, lengths, cols)


def to_f32(a):
    """a float64 numpy array (or None) -> the fp32 torch CPU tensor of the yardstick run"""
    return None if a is None else torch.from_numpy(np.asarray(a, dtype=np.float32))


def yardstick(fn64, fn32):
    """(reference float64 array, max |fp32 torch run - reference|)"""
    ref = fn64()
    got = fn32()
    return ref, float(np.abs(got.double().numpy() - ref).max())


# ---- the guidance of the reference fixtures --------------------------------------------------------------------------------------
FIXTURE_SEED = 29


def fixture_guidance(case: str, B: int, T: int, C: int, levels: int):
    """The terms of fixture ``case`` as fp32 CPU tensors: dict(target, weight, vel, acc, level_scale); absent terms are None.
    Weights are sized for the random-weight models of the fixtures (|x| grows to ~1e3): large enough to move the final sample by far
    more than the parity tolerance, small enough that the explicit steps stay stable (checked when the fixtures are generated)."""
    g = torch.Generator().manual_seed(FIXTURE_SEED)
    Y = torch.randn(B, T, C, generator=g)
    W = torch.zeros(B, T, C)
    for f in (T // 4, T // 2, (3 * T) // 4):           # keyframes on the first 40 and the last 30 columns
        W[:, f, :40] = 0.2
        W[:, f, C - 30:] = 0.2
    W[:, T // 3:T // 3 + 8, 100:120] = 0.05            # a soft target over a stretch of frames
    c = torch.arange(C)
    vel = torch.where(c >= C // 2, torch.tensor(0.03), torch.tensor(0.0))
    acc = torch.where(c < C // 2, torch.tensor(0.01), torch.tensor(0.0))
    out = {"target": Y, "weight": W, "vel": None, "acc": None, "level_scale": None}
    if case in ("plain", "ddpm"):
        out["vel"], out["acc"] = vel, acc
    elif case == "eta":
        out["vel"] = vel
        out["level_scale"] = [1.0 - 0.5 * k / (levels - 1) for k in range(levels)]
    elif case != "harmonize":
        raise ValueError(case)
    return out
