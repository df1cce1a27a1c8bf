"""Plain numpy / torch CPU references, input builders and gates for the small kernels of the sampler (sampler_kernels.hip) and around the
denoiser (rowops.hip).  test_gpu_sampler_ops.py and test_gpu_row_ops.py compare the kernels with them; test_small_ops_ref_cpu.py checks
here, without a GPU, that every reference passes its own gate and that every mutant listed there is rejected on the very inputs the GPU
tests use.  No reference value or gate in this file is taken from a kernel's output.  The one thing read from the library is host code: the
diffusion tables of dsh_diffusion_table, from which the step scalars are rounded as the sampling loop rounds them - so the CPU test needs
the built library too (no GPU).

Philox.  philox4x32_10 is the published Philox4x32-10 (Random123) on uint32 arrays and reproduces its three known answers.  randn_ref
assigns counters and keys as the comment above philox_randn_kernel states them: key = seed, counter = (offset + quad index, 0) for one
stream, (offset + quad index inside the row, row key) for per-row streams, (draw * (row_len * channels / 4) + quad index inside the row,
row key) for ragged rows.  The uniforms ((c >> 8) + 0.5) * 2^-24 are evaluated in float32 (the add rounds for c >> 8 >= 2^23; u = 1.0 is
reachable and gives r = 0), the angle float32(6.2831855) * u2 in float32; r, cos and sin are then taken in float64 from those float32 values.
Gate: |z - z_ref| <= MARGIN * G * 2^-23 * max(r_ref, 2^-23) per element, G = philox_gate_g(): the largest such ratio of the same expression
evaluated wholly in numpy float32, on 2^20 counters at seed 42.  Every Philox mutant is wrong by O(1), six orders above the gate.

Sampler steps.  torch CPU fp32 expressions with one rounded op per reference op (gaussian_diffusion.py:614-622, :993-1056, :464-473,
:598-600, :747-773); the kernels are compared with torch.equal.  NaN inputs are out of scope: the kernel clamps with fminf(fmaxf(.)),
which returns the bound for a NaN, torch.clamp propagates it.

temb.  float64 cos / sin of t * exp(a_j) with a_j the float32 argument chain the kernel documents (-ln(1e4) * j / half, two rounded
float32 ops).  Gate per element: MARGIN * K * 2^-24 (2 t f_j + 1), K = the largest error of torch's fp32 timestep_embedding against ref64 in
units of that scale over all timesteps and frequencies of the test (temb_allow says why not a maximum per row); t = 0 exact.

FiLM fold.  A = gamma * (1 + scale) in two rounded fp32 ops is exact.  B is the kernel's fused multiply-add of beta, the ROUNDED fp32
(1 + scale) and shift: the reference evaluates beta * sc32 + shift in float64 (the product of two fp32 values is exact there) and rounds once;
the gate is 1 fp32 ulp of it (a double rounding can move the float64 value's fp32 rounding off the fused result by one ulp).
"""
import ctypes as C
import functools
import math

import numpy as np
import torch

from bf16_gates import MARGIN  # noqa: F401  (the one margin of every derived gate)

SENTINEL = 12345.0
GUARD = 64                      # sentinel elements behind the last element of every output buffer
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
U64 = 2 ** 64 - 1

KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


# ---- Philox ----------------------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter4, key2, rounds=10, m0=M0, m1=M1, w0=W0, w1=W1):
    """counter4: four uint32 arrays (or scalars) of one shape, key2: two.  Returns the four output words as uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in counter4]
    k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK32 for v in key2)
    for _ in range(rounds):
        p0 = np.uint64(m0) * c[0]
        p1 = np.uint64(m1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK32]
        k0 = (k0 + np.uint64(w0)) & MASK32
        k1 = (k1 + np.uint64(w1)) & MASK32
    return [v.astype(np.uint32) for v in c]


PHILOX_MUTANTS = ("mult_swapped", "weyl_swapped", "nine_rounds", "key_xor", "offset_elems", "low24", "sincos_swapped", "lens_ignored")


def _philox_words(n, seed, offset, row_keys, n_row, row_lens, draw, channels, mutant):
    nquad = (n + 3) // 4
    qd = np.arange(nquad, dtype=np.uint64)
    seed = np.uint64(seed & U64)
    off = np.uint64((offset // 4 if mutant == "offset_elems" else offset) & U64)
    rk = np.zeros(nquad, dtype=np.uint64)
    with np.errstate(over="ignore"):
        if row_keys is None:
            ctr = off + qd
        else:
            rq = np.uint64(n_row // 4)
            b = qd // rq
            inrow = qd - b * rq
            if row_lens is not None and mutant != "lens_ignored":
                adv = np.asarray(row_lens, dtype=np.uint64) * np.uint64(channels) // np.uint64(4)
                ctr = np.uint64(draw) * adv[b.astype(np.int64)] + inrow
            elif row_lens is not None:
                ctr = np.uint64(draw) * rq + inrow
            else:
                ctr = off + inrow
            rk = np.asarray([k & U64 for k in row_keys], dtype=np.uint64)[b.astype(np.int64)]
    key = np.full(nquad, seed, dtype=np.uint64)
    if mutant == "key_xor":
        key, rk = key ^ rk, np.zeros(nquad, dtype=np.uint64)
    kw = {}
    if mutant == "mult_swapped":
        kw = {"m0": M1, "m1": M0}
    elif mutant == "weyl_swapped":
        kw = {"w0": W1, "w1": W0}
    elif mutant == "nine_rounds":
        kw = {"rounds": 9}
    s32 = np.uint64(32)
    return philox4x32_10((ctr & MASK32, ctr >> s32, rk & MASK32, rk >> s32), (key & MASK32, key >> s32), **kw)


def _uniform_angle(words, mutant):
    """(u1, angle) float32 pairs of the two Box-Muller halves of every quad: [nquad, 2] each."""
    bits = [(w & np.uint32(0xFFFFFF)) if mutant == "low24" else (w >> np.uint32(8)) for w in words]
    u = [(b.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24) for b in bits]
    u1 = np.stack([u[0], u[2]], axis=1)
    ang = np.float32(6.2831855) * np.stack([u[1], u[3]], axis=1)
    assert u1.dtype == np.float32 and ang.dtype == np.float32
    return u1, ang


def randn_ref(n, seed, offset=0, row_keys=None, n_row=None, row_lens=None, draw=0, channels=0, mutant=None, with_r=False):
    """float64 [n] standard normals of philox_randn_kernel (with_r: also the Box-Muller radius of every element, for the gate)."""
    assert mutant is None or mutant in PHILOX_MUTANTS
    words = _philox_words(n, seed, offset, row_keys, n_row, row_lens, draw, channels, mutant)
    u1, ang = _uniform_angle(words, mutant)
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    cs, sn = np.cos(ang.astype(np.float64)), np.sin(ang.astype(np.float64))
    if mutant == "sincos_swapped":
        cs, sn = sn, cs
    z = np.stack([r * cs, r * sn], axis=2).reshape(-1)[:n]
    if with_r:
        return z, np.repeat(r.reshape(-1), 2)[:n]
    return z


def randn_f32(n, seed, offset=0):
    """The same expression evaluated wholly in numpy float32 (the calibration of the gate)."""
    u1, ang = _uniform_angle(_philox_words(n, seed, offset, None, None, None, 0, 0, None), None)
    r = np.sqrt(np.float32(-2.0) * np.log(u1))
    z = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=2).reshape(-1)[:n]
    assert z.dtype == np.float32
    return z


def philox_ratio(z, z_ref, r_ref):
    """largest |z - z_ref| / (2^-23 max(r_ref, 2^-23)); NaN / Inf in z give inf"""
    err = np.abs(np.asarray(z, dtype=np.float64) - z_ref) / (2.0 ** -23 * np.maximum(r_ref, 2.0 ** -23))
    return float(np.where(np.isfinite(err), err, np.inf).max()) if err.size else 0.0


@functools.lru_cache(maxsize=1)
def philox_gate_g():
    n = 4 << 20                                        # 2^20 counters
    z_ref, r_ref = randn_ref(n, 42, 0, with_r=True)
    return philox_ratio(randn_f32(n, 42, 0), z_ref, r_ref)


PHILOX_BIG_N = 4 * 524288 + 1029                       # a second trip of the 2048 x 256 grid-stride loop, with a ragged last quad
# (n, seed, offset): tiny and ragged sizes, the carry of the counter's low word, seeds with a high word
PHILOX_CASES = tuple((n, seed, off) for n in (1, 3, 4, 5, 1027) for seed, off in ((42, 0), (42, 1), ((0xDEADBEEF << 32) | 7, 2 ** 32 - 1),
                                                                                 ((1 << 63) | 12345, 2 ** 32 + 5)))
PHILOX_ROW_KEYS = (0, 1, (0xABCD1234 << 32) | 5, (1 << 63) | 99)
RAGGED_T, RAGGED_LENS = 64, (64, 41, 1, 7)


# ---- sampler steps ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table(name, steps=1000, respacing=25):
    from diffsheg_amd import _lib
    buf = (C.c_double * 1024)()
    n = _lib.lib().dsh_diffusion_table(steps, respacing, name.encode(), buf, 1024)
    assert n > 0, name
    return np.array(buf[:n], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def ddim_scalars(k, eta=0.0):
    """(c1, c2, sqrt_ab_prev, sqrt_1m_ab_prev, coef_eps, sigma) of spaced level k as the sampling loop rounds them (sampler.hip): fp64 table
    -> fp32, every further op in fp32."""
    f = np.float32
    c1, c2 = f(_table("sqrt_recip_alphas_cumprod")[k]), f(_table("sqrt_recipm1_alphas_cumprod")[k])
    ab, abp = f(_table("alphas_cumprod")[k]), f(_table("alphas_cumprod_prev")[k])
    sab, s1m = np.sqrt(abp), np.sqrt(f(1) - abp)
    sigma, coef = f(0), s1m
    if eta != 0.0:
        sigma = (f(eta) * np.sqrt((f(1) - abp) / (f(1) - ab))) * np.sqrt(f(1) - ab / abp)
        coef = np.sqrt((f(1) - abp) - sigma * sigma)
        if k == 0:
            sigma = f(0)
    out = tuple(float(v) for v in (c1, c2, sab, s1m, coef, sigma))
    assert all(isinstance(v, np.float32) for v in (c1, c2, sab, s1m, coef, sigma))
    return out


def ddpm_scalars(k):
    """(c1, c2, coef1, coef2, sigma) of level k of the 1000-step chain respaced to 50, as the loop rounds them."""
    f = np.float32
    t = {n: _table(n, 1000, 50) for n in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1",
                                         "posterior_mean_coef2", "posterior_log_variance_clipped")}
    sigma = f(0) if k == 0 else np.exp(f(0.5) * f(t["posterior_log_variance_clipped"][k]))
    return tuple(float(f(v)) for v in (t["sqrt_recip_alphas_cumprod"][k], t["sqrt_recipm1_alphas_cumprod"][k], t["posterior_mean_coef1"][k],
                                       t["posterior_mean_coef2"][k], sigma))


def undo_scalars(k):
    beta = np.float32(_table("betas")[k])
    return float(np.sqrt(np.float32(1) - beta)), float(np.sqrt(beta))


def _t(v):
    return torch.tensor(v, dtype=torch.float32)


def _ab_cd(a, b, c, d, contract, sign=1.0):
    """a * b + sign * c * d: three rounded fp32 ops, or (contract) evaluated in float64 and rounded once"""
    if contract:
        return (a.double() * b.double() + sign * (c.double() * d.double())).float()
    return a * b + c * d if sign > 0 else a * b - c * d


STEP_SITES = ("x0", "mean", "noise1", "gt", "fade")
DDIM_MUTANTS = tuple("contract_" + s for s in STEP_SITES) + ("coef_is_s1m", "linspace_one_sided", "clip_after_eps", "tail_before_select",
                                                            "window_lo+1", "window_hi-1")


def window(prev, new, c_lo, c_hi):
    """what a launch restricted to channels [c_lo, c_hi) leaves in a buffer that held prev (0, 0 = all channels)"""
    if c_hi <= c_lo:
        return new
    out = prev.clone()
    out[..., c_lo:c_hi] = new[..., c_lo:c_hi]
    return out


def linspace01(L, one_sided=False):
    if not one_sided:
        return torch.linspace(0, 1, L)
    return torch.zeros(1) if L == 1 else (_t(1.0) / _t(float(L - 1))) * torch.arange(L, dtype=torch.float32)


def ddim_step_ref(x, eps, sc, noise1=None, clip=0, mask=None, gt=None, nz2=None, L=0, blend=0, tail_blend=0, tail_in=None, mutant=None):
    """One fused DDIM step on all channels: (x_new, x0, tail) with tail = the last L frames of x_new.  sc = ddim_scalars()."""
    c1, c2, sab, s1m, coef, sigma = (_t(v) for v in sc)
    m = mutant or ""
    c1x = c1 * x
    x0 = _ab_cd(c1, x, c2, eps, m == "contract_x0", -1.0)
    if clip and m != "clip_after_eps":
        x0 = x0.clamp(-1.0, 1.0)
    e2 = (c1x - x0) / c2
    if clip and m == "clip_after_eps":
        x0 = x0.clamp(-1.0, 1.0)
    s = _ab_cd(x0, sab, s1m if m == "coef_is_s1m" else coef, e2, m == "contract_mean")
    if noise1 is not None:
        s = (s.double() + sigma.double() * noise1.double()).float() if m == "contract_noise1" else s + sigma * noise1
    out = s
    if mask is not None:
        if tail_in is not None:
            g = gt.clone()
            g[:, :L] = tail_in
        else:
            g = _ab_cd(sab, gt, s1m, nz2, m == "contract_gt")
        if blend and L > 0:
            w = linspace01(L, m == "linspace_one_sided").view(1, -1, 1)
            g = g.clone()
            head = _ab_cd(g[:, :L], 1 - w, s[:, :L], w, m == "contract_fade")
            if tail_blend:
                wr = w.flip(1)
                g[:, -L:] = _ab_cd(g[:, -L:], 1 - wr, s[:, -L:], wr, m == "contract_fade")
            g[:, :L] = head
        out = torch.where(mask, g, s)
    T = x.shape[1]
    tail = (s if m == "tail_before_select" else out)[:, T - L:].clone()
    return out, x0, tail


def ddim_expect(full, prev, c_lo, c_hi, mutant=None):
    """(x, x0_out, tail_out) buffers after a launch on channels [c_lo, c_hi): full = ddim_step_ref(), prev = what the three buffers held."""
    if c_hi > c_lo and mutant == "window_lo+1":
        c_lo += 1
    if c_hi > c_lo and mutant == "window_hi-1":
        c_hi -= 1
    return tuple(window(p, f, c_lo, c_hi) for p, f in zip(prev, full))


DDPM_MUTANTS = ("contract_x0", "contract_mean", "contract_noise", "clip_after_mean")


def ddpm_step_ref(x, eps, noise, sc, clip=0, mutant=None):
    c1, c2, k1, k2, sigma = (_t(v) for v in sc)
    m = mutant or ""
    x0 = _ab_cd(c1, x, c2, eps, m == "contract_x0", -1.0)
    if clip and m != "clip_after_mean":
        x0 = x0.clamp(-1.0, 1.0)
    mean = _ab_cd(k1, x0, k2, x, m == "contract_mean")
    if clip and m == "clip_after_mean":
        x0 = x0.clamp(-1.0, 1.0)
    out = (mean.double() + sigma.double() * noise.double()).float() if m == "contract_noise" else mean + sigma * noise
    return out, x0


def undo_step_ref(x, noise, sc, mutant=None):
    sa, sb = (_t(v) for v in sc)
    return _ab_cd(sa, x, sb, noise, mutant == "contract")


STEP_B, STEP_T, STEP_C, STEP_SPLIT = 3, 24, 232, 103       # SHOW: 103 expression channels in front of 129 gesture channels
STEP_LS = (1, 2, 4, 10)
STEP_WINDOWS = ((0, 0), (STEP_SPLIT, STEP_C), (0, STEP_SPLIT))
STEP_BIG = (10, 240, 232)                                   # 556 800 values: more than the 2048 x 256 grid covers in one trip
# eta mode -> (spaced level, eta, noise1 given)
ETA_MODES = {"eta0": (1, 0.0, False), "eta": (12, 0.5, True), "eta_last": (0, 0.5, True)}


def step_inputs(L, shape=(STEP_B, STEP_T, STEP_C)):
    B, T, Cc = shape
    g = torch.Generator().manual_seed(1000 + L + B)
    t = {n: torch.randn(B, T, Cc, generator=g) for n in ("x", "eps", "gt", "nz1", "nz2")}
    t["tail_in"] = torch.randn(B, L, Cc, generator=g)
    head = torch.zeros(B, T, Cc, dtype=torch.bool)
    head[:, :L] = True
    t["masks"] = {"none": None, "head": head, "dense": torch.rand(B, T, Cc, generator=g) < 0.5}
    return t


def step_combos():
    """(eta mode, clip, mask kind, blend, tail_blend, tails) of the full product; tails = tail_in (with a mask) and tail_out"""
    return [(e, clip, mk, bl, tb, tails) for e in ETA_MODES for clip in (0, 1) for mk in ("none", "head", "dense")
            for (bl, tb) in ((0, 0), (1, 0), (1, 1)) for tails in (0, 1)]


def ddim_case_ref(t, L, combo, mutant=None):
    e, clip, mk, bl, tb, tails = combo
    k, eta, has_n1 = ETA_MODES[e]
    mask = t["masks"][mk]
    return ddim_step_ref(t["x"], t["eps"], ddim_scalars(k, eta), noise1=t["nz1"] if has_n1 else None, clip=clip, mask=mask, gt=t["gt"],
                         nz2=t["nz2"], L=L, blend=bl if mask is not None else 0, tail_blend=tb if mask is not None else 0,
                         tail_in=t["tail_in"] if (tails and mask is not None) else None, mutant=mutant)


# ---- temb ------------------------------------------------------------------------------------------------------------------------------
TEMB_T = tuple(range(1000)) + (10 ** 6,)
TEMB_DIMS = (512, 128)


def temb_ref64(t, dim, mutant=None):
    half = dim // 2
    j = torch.arange(half, dtype=torch.float32)
    arg = torch.tensor(-9.210340371976184, dtype=torch.float32) * j / float(half - 1 if mutant == "half_minus_1" else half)
    assert arg.dtype == torch.float32
    a = torch.as_tensor(t, dtype=torch.float64)[:, None] * torch.exp(arg.double())[None, :]
    return torch.cat([torch.cos(a), torch.sin(a)], dim=1)


def temb_f32(t, dim):
    """timestep_embedding (models/transformer.py:42-59) as torch evaluates it in fp32"""
    half = dim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float32) / half)
    a = torch.as_tensor(t).float()[:, None] * freqs[None, :]
    return torch.cat([torch.cos(a), torch.sin(a)], dim=1)


def temb_scale(t, dim):
    """[len(t), dim] size of one fp32 rounding step of the chain at every element: the frequency f carries a relative error of order 2^-24
    (expf is not correctly rounded, on either side), which the timestep turns into 2^-24 a in the angle a = t f; the product t f is rounded
    to fp32, another 2^-24 a; cos / sin have slope <= 1 and are themselves rounded to fp32 near 1: 2^-24 (2 a + 1)."""
    half = dim // 2
    j = torch.arange(half, dtype=torch.float32)
    arg = torch.tensor(-9.210340371976184, dtype=torch.float32) * j / float(half)
    a = (torch.as_tensor(t, dtype=torch.float64)[:, None] * torch.exp(arg.double())[None, :]).abs()
    return 2.0 ** -24 * (2 * torch.cat([a, a], dim=1) + 1)


@functools.lru_cache(maxsize=None)
def temb_k(dim):
    """the calibration: the largest error of torch's fp32 formula in units of temb_scale, over ALL of TEMB_T x dim (0.86 / 0.91)"""
    t = list(TEMB_T)
    return float(((temb_f32(t, dim).double() - temb_ref64(t, dim)).abs() / temb_scale(t, dim)).max())


def temb_allow(t, dim):
    """[len(t), dim]: MARGIN x temb_k x temb_scale.  ONE constant calibrated over the whole population of timesteps and frequencies, scaled per
    element by the arithmetic.  A maximum of torch's error inside each timestep's row would not be a bound: a row's large angles are its first
    few frequencies only (f_0 = 1 is exact), so such a maximum runs over three to six samples of the rounding of t f, and an expf that returns
    the other neighbour of a near-tie (f_1 at dim 128 lies 0.472 ulp above its rounded value) rounds t f differently.  t = 0 must be exact
    (cos 0, sin 0); the tests assert that beside the gate."""
    return MARGIN * temb_k(dim) * temb_scale(t, dim)


# ---- cfg_mix ---------------------------------------------------------------------------------------------------------------------------
def cfg_inputs(w, B=3, T=5, ld_extra=0, c0=0, per_clip=True, scales=(1.0, 1.15, 0.0)):
    g = torch.Generator().manual_seed(w * 3 + c0 + ld_extra)
    Mc = B * T
    cond_row0 = Mc + 7
    t = {"w": w, "B": B, "T": T, "Mc": Mc, "cond_row0": cond_row0, "c0": c0, "ldo": w + ld_extra, "lde": c0 + w + ld_extra,
         "ldx": c0 + w + ld_extra, "ldx0": w + ld_extra}
    t["o"] = torch.randn(cond_row0 + Mc, t["ldo"], generator=g)
    t["x"] = torch.randn(Mc, t["ldx"], generator=g)
    t["scale"] = torch.tensor(scales[:B] if per_clip else scales[:1], dtype=torch.float32)
    t["scale_row"] = 1 if per_clip else 0
    t["c1"] = 1.0 + torch.rand(B, generator=g)
    t["c2"] = torch.rand(B, generator=g) + 0.1
    return t


def cfg_mix_ref(t, has_null=1, mutant=None):
    """(eps columns [c0, c0 + w), x0 [Mc, w]) in torch fp32"""
    w, Mc, T = t["w"], t["Mc"], t["T"]
    u, k = t["o"][:Mc, :w], t["o"][t["cond_row0"]:t["cond_row0"] + Mc, :w]
    b = torch.arange(Mc) // T
    if has_null:
        s = t["scale"][b * t["scale_row"]][:, None]
        mix = u + s * (k - u)
        e = mix if mutant == "no_shortcut" else torch.where(s == 1.0, k, mix)
    else:
        e = u.clone()
    x0 = t["c1"][b][:, None] * t["x"][:, t["c0"]:t["c0"] + w] - t["c2"][b][:, None] * e
    return e, x0


# ---- data movement ---------------------------------------------------------------------------------------------------------------------
def im2col3_ref(x, lens=None):
    """x [B, T, Cin] -> [B T, 3 Cin]; frames >= lens[b] read as zero by selection"""
    B, T, Cin = x.shape
    out = torch.zeros(B, T, 3, Cin, dtype=x.dtype)
    for b in range(B):
        n = T if lens is None else int(lens[b])
        for tap in range(3):
            lo, hi = max(0, 1 - tap), min(T, n + 1 - tap)        # t + tap - 1 in [0, n)
            if hi > lo:
                out[b, lo:hi, tap] = x[b, lo + tap - 1:hi + tap - 1]
    return out.reshape(B * T, 3 * Cin)


def rne_bf16(x):
    return x.float().bfloat16()


def seed_stream_ref(h0, c, has_null, row1):
    """fp32 stream [R, D] (R = (row1 if has_null else 0) + round_up(Mc, 32)), rows no clip owns 0"""
    Mc, D = h0.shape
    R = (row1 if has_null else 0) + (Mc + 31) // 32 * 32
    h = torch.zeros(R, D)
    h[:Mc] = h0 + c if has_null else h0
    if has_null:
        h[row1:row1 + Mc] = h0
    return h


def pack_expr_ref(src, B, T, ld, lens=None):
    """x0 [B T, ld]: the E columns of src, zero behind them and on frames >= lens[b]"""
    E = src.shape[1]
    x0 = torch.zeros(B * T, ld)
    x0[:, :E] = src
    if lens is not None:
        x0 = x0.view(B, T, ld).clone()
        for b in range(B):
            x0[b, int(lens[b]):] = 0.0
        x0 = x0.view(B * T, ld)
    return x0


# ---- FiLM ------------------------------------------------------------------------------------------------------------------------------
def film_inputs(B, nblk, D, ld_extra=0, n_src=None):
    g = torch.Generator().manual_seed(B * 31 + nblk * 7 + D)
    ld = 2 * D * nblk + ld_extra
    return {"tab": torch.randn(n_src or B, ld, generator=g), "gamma": torch.randn(nblk, D, generator=g), "beta": torch.randn(nblk, D, generator=g),
            "ld": ld, "B": B, "nblk": nblk, "D": D}


def ulp_f32(v):
    a = torch.as_tensor(v, dtype=torch.float64).abs()
    _, e = torch.frexp(a.clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(a), e - 24)


def film_fold_ref(t, idx=None):
    """(A fp32 exact, B float64 -> rounded once to fp32) as [B, nblk, D] each, rows taken through idx"""
    nblk, D = t["nblk"], t["D"]
    rows = t["tab"] if idx is None else t["tab"][torch.as_tensor(idx, dtype=torch.long)]
    r = rows[:, :2 * D * nblk].reshape(rows.shape[0], nblk, 2, D)
    sc = 1.0 + r[:, :, 0]
    A = t["gamma"][None] * sc
    Bc = (t["beta"][None].double() * sc.double() + r[:, :, 1].double()).float()
    return A, Bc


def film_pack(A, Bc, like):
    """[B, nblk, D] pairs back into table rows [B, ld]; columns behind 2 D nblk keep `like`"""
    out = like.clone()
    n = A.shape[0]
    out[:n, :2 * A.shape[1] * A.shape[2]] = torch.stack([A, Bc], dim=2).reshape(n, -1)
    return out


# ---- LayerNorm family (ln_rows with pre_add, ln_film_silu_rows, concat_ln_rows) ----------------------------------------------------------
# Gated as f32_gates.py gates its launches: ref64 = the reference's op sequence in float64, chain32 = the documented expression in float32
# with two-pass row moments in torch's summation order and in the flipped column order; EVERY element within MARGIN x max |chain32 - ref64|,
# the maximum taken over max(M, CAL_ROWS) rows of the same family, the all-constant row of "const" a population of its own.  bf16 outputs:
# that allowance plus half a bf16 ulp of the reference.
LN_DS = (65, 128, 512, 999, 1024)
LN_MS = (1, 5, 77)
LN_FAMILIES = ("plain", "off+50", "lowvar", "const")
CONCAT_WIDTHS = ((33, 16, 8, 8), (512, 256, 128, 0), (512, 256, 128, 103), (512, 256, 128, 128))       # P = 65, 896 (w3 = 0), 999, 1024


def ln_inputs(kind, M, D, family, frames=1, nb=3, film_off=0, bf16_in=False, widths=None):
    """kind "pre": ln_rows with pre_add on the first n_pre rows; "film": ln_film_silu_rows; "concat": concat_ln_rows over `widths` (sum = D,
    segments 1 and 2 in the output's element type when bf16_in)."""
    import f32_gates as F32
    Mc = max(M, F32.CAL_ROWS)
    g = torch.Generator().manual_seed(F32._seed("ln", kind, M, D, family, frames, nb, film_off, bf16_in))
    x = F32.family_rows(family, Mc, D, g, M)
    t = {"kind": kind, "M": M, "D": D, "family": family, "frames": frames, "nb": nb, "film_off": film_off, "bf16_in": bf16_in, "widths": widths,
         "gamma": 1 + 0.3 * torch.randn(D, generator=g), "beta": 0.3 * torch.randn(D, generator=g)}
    t["special"] = [F32.const_row(M)] if family == "const" else []
    if kind == "pre":
        t["pre_add"], t["n_pre"] = 0.5 * torch.randn(D, generator=g), (M + 1) // 2
        t["h_in"] = x
        if family == "const" and M > 1:                                  # the constant row in front takes pre_add: a second one behind n_pre stays constant
            x[M - 1] = x[M - 1, 0].item()
            t["special"].append(M - 1)
        x = x.clone()
        x[:t["n_pre"]] = x[:t["n_pre"]] + t["pre_add"]                  # one fp32 add: what h must hold afterwards, bit for bit
    elif kind == "film":
        film = torch.full((nb, film_off + 2 * D + 8), float("nan"))
        film[:, film_off:film_off + 2 * D] = 0.5 * torch.randn(nb, 2 * D, generator=g)
        t["film"], t["clip"] = film, (torch.arange(Mc) // frames) % nb
        if bf16_in:
            x = rne_bf16(x).float()
    elif kind == "concat" and bf16_in:
        w0, w1, w2, _ = widths
        x[:, w0:w0 + w1 + w2] = rne_bf16(x[:, w0:w0 + w1 + w2]).float()
    t["X"] = x
    return t


def _ln_chain(t, dt, flip=False):
    x, D = t["X"].to(dt), t["D"]
    xs = x.flip(1) if flip else x
    mean = xs.sum(-1, keepdim=True) / D
    var = ((xs - mean) ** 2).sum(-1, keepdim=True) / D
    y = (x - mean) * (1 / torch.sqrt(var + 1e-5)) * t["gamma"].to(dt) + t["beta"].to(dt)
    if t["kind"] == "film":
        f = t["film"].to(dt)[t["clip"]][:, t["film_off"]:t["film_off"] + 2 * D]
        y = torch.nn.functional.silu(y * (1 + f[:, :D]) + f[:, D:])
    return y


def ln_ref64(t):
    D = t["D"]
    y = torch.nn.functional.layer_norm(t["X"].double(), (D,), t["gamma"].double(), t["beta"].double(), 1e-5)
    if t["kind"] == "film":
        f = t["film"].double()[t["clip"]][:, t["film_off"]:t["film_off"] + 2 * D]
        y = torch.nn.functional.silu(y * (1 + f[:, :D]) + f[:, D:])
    return y


def const_row_slack(t, r):
    """An all-constant row c: the exact result is beta, and what an evaluation returns is (c - mean) eps^-1/2 gamma + beta with whatever
    rounding error its sum of D equal terms left in the mean - zero in torch's order for some c (the calibration of that one row is then 0),
    not zero in another.  rowops.hip documents its order: one 64-lane wave per row, lane-strided partial sums (ceil(D / 64) terms each) and a
    6-step butterfly, so at most h = ceil(D / 64) + 6 roundings of relative size 2^-24 on the way: |mean - c| <= h 2^-24 |c|.  Behind the
    FiLM + SiLU front the same times max |1 + scale| and the SiLU's Lipschitz constant 1.1.  Zero for a row that is not constant."""
    x = t["X"][r]
    if float(x.max()) != float(x.min()):
        return 0.0
    D = t["D"]
    h = (D + 63) // 64 + 6
    s = h * 2.0 ** -24 * float(x.abs().max()) * 1e-5 ** -0.5 * float(t["gamma"].abs().max())
    if t["kind"] == "film":
        f = t["film"][t["clip"][r], t["film_off"]:t["film_off"] + D]
        s *= 1.1 * float((1 + f.double()).abs().max())
    return s


def ln_gate(t):
    """(ref64 [rows, D], allowance [rows, 1], calibration maximum) over all calibration rows"""
    if "_gate" not in t:
        ref = ln_ref64(t)
        err = torch.maximum(*((_ln_chain(t, torch.float32, flip).double() - ref).abs() for flip in (False, True)))
        rest = torch.ones(err.shape[0], dtype=torch.bool)
        rest[t["special"]] = False
        cal = float(err[rest].max())
        allow = torch.full((err.shape[0], 1), MARGIN * cal, dtype=torch.float64)
        for r in t["special"]:
            allow[r] = MARGIN * float(err[r].max()) + const_row_slack(t, r)
        t["_gate"] = (ref, allow, cal)
    return t["_gate"]


def ln_check(t, out, what):
    """out [M, D] fp32 or bf16 against the gate; returns the largest |out - ref64| / calibration of its row"""
    import bf16_gates as BG
    ref, allow, cal = ln_gate(t)
    M = t["M"]
    a = allow[:M].expand(M, t["D"])
    if out.dtype == torch.bfloat16:
        return BG.assert_rounded(out, ref[:M], slack=a, what=what, frames=t["frames"], nb=t["nb"])
    BG.assert_close_f32(out, ref[:M], a, what, frames=t["frames"], nb=t["nb"])
    return float(((out.double() - ref[:M]).abs() / allow[:M].clamp_min(1e-300)).max()) * MARGIN
