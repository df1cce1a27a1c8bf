"""CPU restatements for few-step sampling (free timestep subsets, the DPM-Solver++(2M) step): tables of a kept list through the oracle's
``diffusion_tables``, the oracle's own ``ddim_step`` / ``undo_step``, a fp32 torch ``dpm2m_step`` in the kernel's operation order, the loop
with the order rule, and float64 restatements of the solver coefficients and of both solvers on a problem with a closed-form answer.

Test infrastructure only; never imported by the product path."""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from oracle import sampler_ref as S

LOGSNR8 = [0, 8, 44, 177, 440, 673, 851, 999]
LOGSNR10 = [0, 5, 22, 73, 202, 410, 603, 757, 886, 999]


# ----------------------------------------------------------------------------- subsets and tables
def kept_tables(n: int, kept: Sequence[int]):
    """respace.py:68-82 for an arbitrary ascending list of original timesteps."""
    base = S.diffusion_tables(S.linear_betas(n))["alphas_cumprod"]
    last, nb = 1.0, []
    for t in kept:
        nb.append(1.0 - base[t] / last)
        last = base[t]
    return S.diffusion_tables(np.array(nb)), list(kept)


def half_logsnr(a):
    return 0.5 * np.log(a / (1.0 - a))


def logsnr_timesteps(n: int, k: int) -> List[int]:
    """k timesteps uniform in lambda = log(ac / (1 - ac)) / 2: nearest timestep per grid point, ties to the lower one."""
    lam = half_logsnr(S.diffusion_tables(S.linear_betas(n))["alphas_cumprod"])
    kept = sorted(int(np.argmin(np.abs(lam - g))) for g in np.linspace(lam[-1], lam[0], k))
    if len(set(kept)) != k:
        raise ValueError(f"{len(set(kept))} distinct")
    return kept


def section_timesteps(n: int, counts: Sequence[int]) -> List[int]:
    """Section counts (respace.py:35-57) restated: evenly spaced (running float sum, rounded) steps from each equal portion."""
    size_per, extra = divmod(n, len(counts))
    start, out = 0, []
    for i, c in enumerate(counts):
        size = size_per + (1 if i < extra else 0)
        if size < c:
            raise ValueError(f"cannot divide section of {size} steps into {c}")
        stride, cur = (1 if c <= 1 else (size - 1) / (c - 1)), 0.0
        for _ in range(c):
            out.append(start + round(cur))
            cur += stride
        start += size
    return sorted(set(out))


def solver_coeffs64(tb, k: int):
    """(A, Bc, G) at spaced level k in float64; G = 0 where there is no second-order step (k = 0, the top level)."""
    ac = tb["alphas_cumprod"]
    ab, abp = ac[k], tb["alphas_cumprod_prev"][k]
    with np.errstate(divide="ignore"):
        h = half_logsnr(abp) - half_logsnr(ab)
    A = np.sqrt((1.0 - abp) / (1.0 - ab))
    Bc = -np.sqrt(abp) * np.expm1(-h)
    G = 0.0 if (k == 0 or k + 1 >= len(ac)) else h / (2.0 * (half_logsnr(ab) - half_logsnr(ac[k + 1])))
    return float(A), float(Bc), float(G)


def masked_start_level(n: int, kept: Sequence[int]) -> int:
    """t_T of a masked window on a subset that is no stride: one past the first level at or below alphas_cumprod[14] of ddim25."""
    at = S.spaced_tables(n, "ddim25")[0]["alphas_cumprod"][14]
    ac = kept_tables(n, kept)[0]["alphas_cumprod"]
    hit = [k for k in range(len(ac)) if ac[k] <= at]
    return (hit[0] + 1) if hit else len(ac)


def jump_schedule_from(t_T: int, jump_length: int, jump_n_sample: int) -> List[int]:
    """scheduler.py:178-208 walked from a given t_T."""
    jumps = {j: jump_n_sample - 1 for j in range(0, t_T - jump_length, jump_length)}
    t, ts = t_T, []
    while t >= 1:
        t -= 1
        ts.append(t)
        if jumps.get(t, 0) > 0:
            jumps[t] -= 1
            for _ in range(jump_length):
                t += 1
                ts.append(t)
    ts.append(-1)
    return ts


# ----------------------------------------------------------------------------- the fp32 step, in the kernel's operation order
def _f32(v) -> torch.Tensor:
    return torch.tensor(np.float32(v))


def linspace01(L: int) -> torch.Tensor:
    """torch.linspace(0, 1, L) in fp32 (what the DDIM step's fade uses)."""
    return torch.linspace(0, 1, L)


def dpm2m_step(x, eps, x0_prev, c1, c2, A, Bc, G, sab=None, s1m=None, mask=None, gt=None, nz2=None, L=0, blend=0, tail_blend=0, clip=0):
    """x0 = c1 x - c2 eps (clamped when clip); D = x0 + G (x0 - x0_prev); s = A x + Bc D; then the RePaint branch of the DDIM step.  Every
    product and sum is one rounded fp32 torch op; scalars are fp32 tensors.  Returns (new x, x0)."""
    c1, c2, A, Bc, G = (_f32(v) for v in (c1, c2, A, Bc, G))
    x0 = c1 * x - c2 * eps
    if clip:
        x0 = x0.clamp(-1, 1)
    D = x0 + G * (x0 - x0_prev)
    s = A * x + Bc * D
    if mask is not None:
        g = _f32(sab) * gt + _f32(s1m) * nz2
        if blend and L > 0:
            T = x.shape[1]
            w = linspace01(L).view(1, -1, 1)
            g = g.clone()
            g[:, :L] = g[:, :L] * (1 - w) + s[:, :L] * w
            if tail_blend:
                wr = w.flip(1)
                g[:, T - L:] = g[:, T - L:] * (1 - wr) + s[:, T - L:] * wr
        s = torch.where(mask.bool(), g, s)
    return s, x0


def ddim_step_f32(x, eps, c1, c2, sab, s1m):
    """The unmasked DDIM step at eta = 0 from explicit fp32 scalars, for bit-for-bit comparisons: the oracle's ``ddim_step`` takes
    ``sqrt(1 - ab_prev)`` with torch.sqrt on a 0-dim tensor, which is not correctly rounded on every host CPU (seen 1 ulp off sqrtf at
    level 9 of logsnr10), while the native loop and ``step_scalars`` use the correctly rounded fp32 square root.  Returns (new x, x0)."""
    c1, c2, sab, s1m = (_f32(v) for v in (c1, c2, sab, s1m))
    c1x = c1 * x
    x0 = c1x - c2 * eps
    return x0 * sab + s1m * ((c1x - x0) / c2), x0


def window(prev, new, c_lo, c_hi):
    if c_hi <= c_lo:
        return new
    out = prev.clone()
    out[..., c_lo:c_hi] = new[..., c_lo:c_hi]
    return out


def step_scalars(tb, k: int):
    """fp32 scalars of a step at level k, as the native loop rounds them: c1, c2 (fp64 table -> fp32), sqrt(ab_prev), sqrt(1 - ab_prev)
    (fp32 sqrt of the fp32 table value), A, Bc, G (fp64 -> fp32)."""
    c1, c2 = np.float32(tb["sqrt_recip_alphas_cumprod"][k]), np.float32(tb["sqrt_recipm1_alphas_cumprod"][k])
    abp = np.float32(tb["alphas_cumprod_prev"][k])
    sab, s1m = np.sqrt(abp), np.sqrt(np.float32(1.0) - abp)
    A, Bc, G = (np.float32(v) for v in solver_coeffs64(tb, k))
    return float(c1), float(c2), float(sab), float(s1m), float(A), float(Bc), float(G)


# ----------------------------------------------------------------------------- the loop with the order rule
def sample_loop(eps_fn, shape, y: Optional[dict], noise: S.NoiseSource, kept: Sequence[int], *, n_steps=1000, solver="dpm2m",
                times: Optional[Sequence[int]] = None, overlap_len=10, add_blend=True, clip_denoised=False, trace: Optional[list] = None,
                x_init=None):
    """The DDIM loop of the oracle on a kept list, with the DPM-Solver++(2M) update where the order rule allows it: a denoise step at level
    k is second order iff the previous executed step was the denoise step at level k + 1 and k != 0.  Draws: those of the DDIM loop
    (x_T; per denoise step the randn_like, then the gt noise when masked; per undo step one).  ``times``: the masked schedule (levels,
    ending in -1); None: the plain loop."""
    tb, tmap = kept_tables(n_steps, kept)
    x = noise.randn(shape) if x_init is None else x_init
    masked = bool(y) and "outpainting_mask" in y and bool(y["outpainting_mask"].any())
    if times is None:
        plan = [("denoise", k) for k in range(len(tmap) - 1, -1, -1)]
    else:
        plan = [("denoise" if b < a else "undo", a) for a, b in zip(times[:-1], times[1:])]
    last, x0_prev = -1, None
    for kind, k in plan:
        if kind == "undo":
            x = S.undo_step(tb, k, x, noise)
            last = -1
            if trace is not None:
                trace.append(("undo", k, x.clone(), None))
            continue
        eps = S._call(eps_fn, tb, tmap, k, x)
        if solver == "dpm2m" and k != 0 and last == k + 1:
            c1, c2, sab, s1m, A, Bc, G = step_scalars(tb, k)
            noise.randn(shape)                                   # the step's randn_like: drawn, unused at eta = 0
            kw = {}
            if masked:
                nz2 = noise.randn(shape)
                kw = dict(sab=sab, s1m=s1m, mask=y["outpainting_mask"], gt=y["gt"], nz2=nz2, L=overlap_len,
                          blend=int(s1m < 0.2 and add_blend))
            x, x0 = dpm2m_step(x, eps, x0_prev, c1, c2, A, Bc, G, clip=int(clip_denoised), **kw)
        else:
            x, x0 = S.ddim_step(tb, k, x, eps, y if masked else None, noise, overlap_len, add_blend, clip_denoised)
        x0_prev, last = x0, k
        if trace is not None:
            trace.append(("denoise", k, x.clone(), x0.clone()))
    return x


# ----------------------------------------------------------------------------- float64: a problem with a closed-form answer
def analytic_errors(kept: Sequence[int], s: float, solver: str, n_steps: int = 1000) -> float:
    """Data ~ N(0, s^2): eps(x, k) = sigma_k x / (ac_k s^2 + 1 - ac_k) and the exact ODE solution from the top level is
    x_T sqrt(s^2 / (ac_top s^2 + 1 - ac_top)).  Everything is linear in x_T: returns |final - exact| for x_T = 1, in float64."""
    tb, _ = kept_tables(n_steps, kept)
    ac, acp = tb["alphas_cumprod"], tb["alphas_cumprod_prev"]
    K = len(ac)
    x, x0_prev, last = 1.0, None, -1
    for k in range(K - 1, -1, -1):
        eps = np.sqrt(1.0 - ac[k]) * x / (ac[k] * s * s + 1.0 - ac[k])
        x0 = (x - np.sqrt(1.0 - ac[k]) * eps) / np.sqrt(ac[k])
        if solver == "dpm2m" and k != 0 and last == k + 1:
            A, Bc, G = solver_coeffs64(tb, k)
            x = A * x + Bc * (x0 + G * (x0 - x0_prev))
        else:
            x = np.sqrt(acp[k]) * x0 + np.sqrt(1.0 - acp[k]) * eps
        x0_prev, last = x0, k
    exact = np.sqrt(s * s / (ac[K - 1] * s * s + 1.0 - ac[K - 1]))
    return abs(x - exact)
