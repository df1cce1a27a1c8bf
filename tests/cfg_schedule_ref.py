"""CPU emulation of the scheduled classifier-free mix (rowops.hip cfg_mix_sched_kernel / cfg_rescale_kernel; include/diffsheg_hip.h
dsh_set_guidance_schedule states the formulas): the mix in torch fp32, one rounding per operation like the kernel's, the rescale statistics
in fp64 numpy.  With every gain 1 and phi 0 it is small_ops_ref.cfg_mix_ref.

Per clip b, at its model timestep t_b, reading row `which` of the table:
    s_eff = g == 1 ? s : 1 + g (s - 1)            g = table[which][clamp(t_b)], s = scale[b]
    e     = s_eff == 1 ? k : u + s_eff (k - u)
    f     = float32(phi sigma_k / sigma_e + (1 - phi))   over the clip's len_b x w valid elements, unbiased, fp64; 1 where s_eff == 1,
            n < 2 or sigma_e is not finite and positive
    e'    = f e,  x0 = c1 x - c2 e'

MUTANTS are the wrong readings of that definition which the tests must be able to tell from it."""
import numpy as np
import torch

import small_ops_ref as R

MUTANTS = ("gain_on_s", "no_gain_shortcut", "stats_padded", "stats_all_channels", "x0_unrescaled")

# gains and scales of the op-level tests; every (gain, scale) pair occurs in PAIRS, three clips at a time
GAINS = (0.0, 1.0, 0.5, 2.5, -1.0)
SCALES = (1.0, 1.25, 0.0, 2.0)
TABLE = torch.tensor([[0.0, 1.0, 0.5, 2.5, -1.0, 1.0, 0.5],
                      [2.5, -1.0, 1.0, 0.0, 0.5, 0.0, 2.5]], dtype=torch.float32)     # [2, n_steps = 7]; row 0 begins with GAINS in order


def round_up(a, b):
    return (a + b - 1) // b * b


def pair_cases():
    """[(scales of the three clips, timesteps of the three clips)] covering GAINS x SCALES through row 0 of TABLE (gain = TABLE[0][t])."""
    pairs = [(s, t) for t in range(len(GAINS)) for s in SCALES]
    pairs += [pairs[0]] * (-len(pairs) % 3)
    return [(tuple(p[0] for p in pairs[i:i + 3]), tuple(p[1] for p in pairs[i:i + 3])) for i in range(0, len(pairs), 3)]


def sched_inputs(w, frames, scales, ts, which=0, phi=0.0, lens=None, ld_extra=3, c0=0, cond_pad=False, table=TABLE, seed=0):
    """small_ops_ref.cfg_inputs' dictionary for B = 3 clips plus the schedule's fields.  cond_pad: the conditional half starts at
    round_up(Mc, 256) (the token-per-lane layout) instead of at Mc."""
    B = 3
    t = R.cfg_inputs(w, B=B, T=frames, ld_extra=ld_extra, c0=c0, per_clip=True, scales=tuple(scales))
    Mc = t["Mc"]
    cond_row0 = round_up(Mc, 256) if cond_pad else Mc
    g = torch.Generator().manual_seed(1000 + 7 * w + frames + seed)
    o = torch.randn(cond_row0 + Mc, t["ldo"], generator=g)
    t.update(cond_row0=cond_row0, o=o, t=torch.tensor(ts, dtype=torch.int64), t_row=1, table=table.clone(), which=which,
             phi=float(np.float32(phi)), lens=None if lens is None else [int(v) for v in lens])
    return t


def s_eff_ref(scale, gain, mutant=None):
    """fp32 tensors [B] -> the effective scale, each operation rounded"""
    s, g = scale.float(), gain.float()
    if mutant == "gain_on_s":
        eff = g * s
    else:
        eff = 1.0 + g * (s - 1.0)
    return eff if mutant == "no_gain_shortcut" else torch.where(g == 1.0, s, eff)


def rescale_factor(k, e, phi):
    """k, e: the clip's valid elements (any shape, fp32) -> f as float32"""
    k64, e64 = k.double().numpy().reshape(-1), e.double().numpy().reshape(-1)
    if k64.size < 2:
        return np.float32(1.0)
    with np.errstate(all="ignore"):
        sk, se = np.std(k64, ddof=1), np.std(e64, ddof=1)
        if not (np.isfinite(se) and se > 0):
            return np.float32(1.0)
        p = np.float64(np.float32(phi))
        return np.float32(p * sk / se + (1.0 - p))


def cfg_mix_sched_ref(t, mutant=None):
    """(eps columns [c0, c0 + w), x0 [Mc, w], f [B]) — eps and x0 in torch fp32; rows t >= len_b of a rescaled clip hold e' too (the kernel
    scales the whole clip), but only valid rows are specified"""
    w, Mc, T, B = t["w"], t["Mc"], t["T"], t["B"]
    ldo = t["ldo"]
    wide = mutant == "stats_all_channels"
    cols = ldo if wide else w
    u, k = t["o"][:Mc, :cols], t["o"][t["cond_row0"]:t["cond_row0"] + Mc, :cols]
    b = torch.arange(Mc) // T
    n_steps = t["table"].shape[1]
    tb = t["t"][torch.arange(B) * t["t_row"]].clamp(0, n_steps - 1)
    gain = t["table"][t["which"]][tb]
    se = s_eff_ref(t["scale"][torch.arange(B) * t["scale_row"]], gain, mutant)
    s = se[b][:, None]
    mix = u + s * (k - u)
    e_all = torch.where(s == 1.0, k, mix)
    e = e_all[:, :w].clone()
    f = np.ones(B, dtype=np.float32)
    e_out = e.clone()
    if t["phi"] > 0:
        for c in range(B):
            if float(se[c]) == 1.0:
                continue
            n = T if (t["lens"] is None or mutant == "stats_padded") else t["lens"][c]
            rows = slice(c * T, c * T + n)
            f[c] = rescale_factor(k[rows], e_all[rows] if wide else e[rows], t["phi"])
            e_out[c * T:(c + 1) * T] = torch.tensor(f[c]) * e[c * T:(c + 1) * T]
    ex = e if mutant == "x0_unrescaled" else e_out
    x0 = t["c1"][b][:, None] * t["x"][:, t["c0"]:t["c0"] + w] - t["c2"][b][:, None] * ex
    return e_out, x0, f


def valid_mask(t):
    """[Mc] bool: the rows t < len_b"""
    T, B = t["T"], t["B"]
    lens = [T] * B if t["lens"] is None else t["lens"]
    return torch.tensor([r % T < lens[r // T] for r in range(t["Mc"])])


def ulp_distance(a, b):
    """|a - b| in units in the last place of fp32 tensors of one sign pattern (ordered-integer distance); inf where either is not finite"""
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    ia = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return (ia - ib).abs()
