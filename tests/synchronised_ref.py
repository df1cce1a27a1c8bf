"""Torch restatement of the synchronised window batches, shared by the CPU and the GPU tests.

`window_sync` is dsh_op_window_sync in eager torch: every product and sum is one rounded fp32 op, in the kernel's order, and the weights
are torch.linspace's own values, so on the device the two agree bit for bit.  `ddim_step` is the eta = 0 DDIM update in the kernel's
operation order; `synchronised_loop` one whole loop (evaluate, step, sync) over any eps function; `shared_pairs` the index pairs of the
frames two windows share."""
import numpy as np
import torch


def window_sync(x, left, L, lens=None, c_lo=0, c_hi=0):
    """A new tensor: x [B, T, C] with, for every row b with p = left[b] >= 0, x[p, n_p - L : n_p] and x[b, :L] both replaced by
    a * (1 - w) + r * w on the columns [c_lo, c_hi) ((0, 0): all); n_p = lens[p] or T."""
    x = x.clone()
    T = x.shape[1]
    w = torch.linspace(0, 1, L, device=x.device, dtype=torch.float32)[:, None]
    cols = slice(None) if c_hi <= c_lo else slice(c_lo, c_hi)
    for b, p in enumerate(left):
        if p < 0:
            continue
        n_p = int(lens[p]) if lens is not None else T
        a, r = x[p, n_p - L:n_p, cols].clone(), x[b, :L, cols].clone()
        v = a * (1 - w) + r * w
        x[p, n_p - L:n_p, cols] = v
        x[b, :L, cols] = v
    return x


def shared_pairs(left, L, lens, T):
    """[(p, slice of p's frames, b, slice of b's frames)] for every row b with a left neighbour p."""
    out = []
    for b, p in enumerate(left):
        if p >= 0:
            n_p = int(lens[p]) if lens is not None else T
            out.append((p, slice(n_p - L, n_p), b, slice(0, L)))
    return out


def copies_equal(x, left, L, lens=None):
    """every shared frame holds the same bits in both of its windows"""
    return all(torch.equal(x[p, sp], x[b, sb]) for p, sp, b, sb in shared_pairs(left, L, lens, x.shape[1]))


def max_copy_gap(x, left, L, lens=None):
    return max([float((x[p, sp] - x[b, sb]).abs().max()) for p, sp, b, sb in shared_pairs(left, L, lens, x.shape[1])] or [0.0])


def ddim_tables(steps=1000, k=25):
    """(alphas_cumprod, alphas_cumprod_prev) of the 'ddimK' stride of the linear schedule, float64 (sampler.hip: linear_betas, make_tables)."""
    scale = 1000.0 / steps
    betas = np.linspace(scale * 1e-4, scale * 0.02, steps, dtype=np.float64)
    ac = np.cumprod(1.0 - betas)
    stride = next(s for s in range(1, steps) if (steps + s - 1) // s == k)
    kept = list(range(0, steps, stride))
    ac_k = ac[kept]
    return ac_k, np.concatenate([[1.0], ac_k[:-1]]), kept


def step_scalars(ac, ac_prev):
    """(c1, c2, sqrt_ab_prev, sqrt_1m_ab_prev) of one level as the sampler rounds them: fp64 table -> fp32, the two square roots of the
    previous level taken in fp32 (sampler.hip, step_consts)."""
    c1, c2 = np.float32(np.sqrt(1.0 / ac)), np.float32(np.sqrt(1.0 / ac - 1.0))
    abp = np.float32(ac_prev)
    return float(c1), float(c2), float(np.sqrt(abp)), float(np.sqrt(np.float32(1) - abp))


def ddim_step(x, eps, c1, c2, sab, s1m):
    """the eta = 0 DDIM update in the kernel's operation order (sampler_kernels.hip, ddim_step_kernel)"""
    c1x = c1 * x
    x0 = c1x - c2 * eps
    e2 = (c1x - x0) / c2
    return x0 * sab + s1m * e2


def synchronised_loop(eps_fn, x_T, left, L, lens=None, k=25, sync=True):
    """x after every step [k, B, T, C]: eps_fn(x, level) -> eps, the DDIM step, then the reconciliation of the shared frames."""
    ac, acp, _ = ddim_tables(1000, k)
    x, trace = x_T.clone(), []
    for lvl in range(k - 1, -1, -1):
        x = ddim_step(x, eps_fn(x, lvl), *step_scalars(ac[lvl], acp[lvl]))
        if sync:
            x = window_sync(x, left, L, lens)
        trace.append(x)
    return torch.stack(trace, 0)
