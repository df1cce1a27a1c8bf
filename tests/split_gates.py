"""Emulation and gates of the split-bf16 main loop (gemm_f32_split.hip, precision "bf16x3"), derived from the arithmetic and never from a
kernel's output (plain torch, CPU).  Operands, fp64 references and the fp32 calibration are those of f32_gates.py: the split loop computes
what gemm_f32_pro.hip computes, with another product.

The loop.  x = hi + lo + r with hi = RNE_bf16(x), lo = RNE_bf16(x - hi): |x - hi| <= 2^-8 |x| (bf16 carries 8 significant bits, half an ulp
is 2^-8 relative at worst) and |r| <= 2^-8 |x - hi| <= 2^-16 |x|.  The product of two such numbers is formed as
    a w ~ a_lo w_hi + a_hi w_lo + a_hi w_hi,
every piece product exact in the fp32 accumulator's input (8 x 8 bits).  Dropped: a_lo w_lo (<= 2^-16 |a w|), r_a w and a r_w (<= 2^-16 |a w|
each): at most 3 x 2^-16 |a w| per product.  PRO 1 splits x - x0 (x0 = the mean of the row's first 32 columns, the kernel's grouping of the
sum, tile_mean()) and evaluates rstd ((x - x0) W'^T - (mean - x0) c) + d; zero-padded columns are split as 0.

emul()       the loop in torch: the RNE pieces in fp32 exactly as the hardware forms them, the three products and everything behind them in
             float64 (so the emulation carries the split error and nothing else).
split_term() the worst case of what the split drops, per output element:
                 PRO 0 / 2   3 x 2^-16 x sum_k |a_k| |W_nk|           (a: the rows the launch stages, behind the front for PRO 2)
                 PRO 1       3 x 2^-16 x rstd x sum_k |x_k - x0| |W'_nk|
             times the Lipschitz constant of the activation behind it (SiLU 1.1, GELU 1.13; bf16_gates.py).
Two gates, both on EVERY element:
  check()       |out - ref64| <= f32_gates allowance (MARGIN x the fp32 chain's own distance from fp64: the accumulation, the moments, the
                SiLU) + split_term().  The DERIVED gate: what the arithmetic allows a split loop.
  check_emul()  |out - emul| <= f32_gates allowance alone.  The PINNING gate: a kernel that forms exactly these three products from exactly
                these RNE pieces differs from emul() by its fp32 accumulation and fp32 fronts only (a kernel's PRO 2 output: plus one
                rounding flip of a lo piece, front_flip()).
The derived gate is a worst case over K aligned remainders; random remainders sit a factor ~sqrt(K) inside it.  So it sees what breaks the
2^-16 order (a dropped term: 2^-8; an unshifted PRO 1 row at offset -200), and it cannot see what stays inside that order (truncated lo
pieces: 2 x 2^-16 per remainder in place of 2^-16) - the pinning gate sees those, wherever the fp32 chain itself is more exact than
2^-16, which is every family but the whole-row offsets.  test_split_gates_cpu.py states which mutant which gate must reject, and where.
"""
import torch
import torch.nn.functional as F

import f32_gates as G
from bf16_gates import GELU_LIP, SILU_LIP, truncate_bf16

F64 = torch.float64
SPLIT_REL = 3 * 2.0 ** -16
_LIP = {0: 1.0, 1: SILU_LIP, 2: GELU_LIP}
FAMILIES = ("plain", "off+50", "off-200", "out300", "out-1e4", "lowvar")      # the issue's families (f32_gates.family_rows)


def split(x, trunc_lo=False):
    """(hi, lo) in fp32: hi = RNE_bf16(x), lo = RNE_bf16(x - hi) (x - hi is exact in fp32); trunc_lo: lo by dropping bits (mutant)."""
    x = x.float()
    hi = x.bfloat16().float()
    d = x - hi
    return hi, (truncate_bf16(d) if trunc_lo else d.bfloat16()).float()


def prod3(a, w, drop_alo=False, trunc_lo=False):
    """[M, N] float64: a_lo w_hi + a_hi w_lo + a_hi w_hi over the rows of a [M, K] and w [N, K] (fp32)"""
    ah, al = split(a, trunc_lo)
    wh, wl = split(w, trunc_lo)
    p = ah.double() @ wl.double().T + ah.double() @ wh.double().T
    return p if drop_alo else p + al.double() @ wh.double().T


def tile_mean(xp):
    """The kernel's x0 in fp32: four staging lanes x eight floats of the first K tile, ((a+b)+(c+d))+((e+f)+(g+h)) per lane, then
    (t0 + t1) + (t2 + t3), times 1/32."""
    v = xp[:, :32].float().reshape(-1, 4, 8)
    t = ((v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])) + ((v[..., 4] + v[..., 5]) + (v[..., 6] + v[..., 7]))
    return ((t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3])) * torch.tensor(1.0 / 32.0)


def pro1_shifted(t, shifted=True):
    """(d [M, K] fp32 = x - x0 on the real columns, 0 on the padded ones; x0 [M] fp32)"""
    xp = t["Xp"]
    x0 = tile_mean(xp) if shifted else torch.zeros(xp.shape[0])
    d = xp - x0[:, None]
    d[:, t["k_real"]:] = 0
    return d, x0


def pro2_rows(t, dt):
    """the rows a PRO 2 launch stages: SiLU(xhat scale' + shift'), two-pass moments, in dt"""
    K, off = t["K"], t["film_off"]
    x = t["X"].to(dt)
    mean, rstd = G.two_pass(x)
    f = t["film"].to(dt)[t["clip"]]
    return F.silu((x - mean) * rstd * f[:, off:off + K] + f[:, off + K:off + 2 * K])


def emul(t, drop_alo=False, trunc_lo=False, shifted=True):
    """The split loop on the operands of an f32_gates case, [rows, N] float64.  The keyword arguments are the mutants."""
    kw = {"drop_alo": drop_alo, "trunc_lo": trunc_lo}
    act = G._ACTS[t["act"]]
    if t["kind"] == "pro0":
        y = act(prod3(t["X"], t["W"], **kw) + t["b"].double())
        return y + t["R"].double() if t["R"] is not None else y
    if t["kind"] == "pro1":
        k = t["k_real"]
        d, _ = pro1_shifted(t, shifted)
        dm = d.double().sum(1, keepdim=True) / k
        var = ((d.double() ** 2).sum(1, keepdim=True) / k - dm ** 2).clamp_min(0)
        rstd = 1 / torch.sqrt(var + G.EPS)
        return act(rstd * (prod3(d, t["Wf"], **kw) - dm * t["fc"].double()) + t["fd"].double())
    if t["kind"] == "pro2":
        y = prod3(pro2_rows(t, torch.float32), t["W"], **kw) + t["b"].double()
        return y + t["R"].double() if t["R"] is not None else y
    raise ValueError(t["kind"])


def split_term(t):
    """[rows, N] float64: the worst case of the dropped terms (module docstring)"""
    if "_split" not in t:
        if t["kind"] == "pro0":
            s = t["X"].double().abs() @ t["W"].double().abs().T
        elif t["kind"] == "pro1":
            d, _ = pro1_shifted(t)
            _, rstd = G.two_pass(t["X"].double())
            s = rstd * (d.double().abs() @ t["Wf"].double().abs().T)
        elif t["kind"] == "pro2":
            s = pro2_rows(t, F64).abs() @ t["W"].double().abs().T
        else:
            raise ValueError(t["kind"])
        t["_split"] = SPLIT_REL * _LIP[t["act"]] * s
    return t["_split"]


def _emul_cached(t):
    if "_emul" not in t:
        t["_emul"] = emul(t)
    return t["_emul"]


def _rows_of(t, out):
    rows = G.valid_rows(t)
    return rows, out.detach().cpu().reshape(-1, t["N"])[:len(rows)]


def check(t, out, what=None):
    """The derived gate.  Returns the largest |out - ref64| / allowance."""
    ref, allow, _ = G.gate(t)
    rows, o = _rows_of(t, out)
    a = allow[rows] + split_term(t)[rows]
    G.assert_close_f32(o, ref[rows], a, what or f"{t.get('name', t['kind'])} (derived gate)", frames=t.get("frames", 0), nb=t.get("nb", 0))
    return float(((o.double() - ref[rows]).abs() / a.clamp_min(1e-300)).max())


def front_flip(t):
    """[rows, N]: one worst-placed rounding flip of a lo piece of a PRO 2 row.  The rows a PRO 2 launch splits come out of an fp32 front
    (one-pass moments, hardware exp and rcp in the SiLU) that no CPU evaluation reproduces bit for bit; where two fronts differ by an fp32
    ulp next to a rounding boundary of lo, lo moves by one of ITS ulps, ulp_bf16(lo) <= 2^-7 |lo| <= 2^-15 |s| (hi moving is made up by lo).
    One flip per output, met by the row's largest weight, as bf16_gates.flip_bound: at K = 32 it is of the size of the fp32 allowance, at
    K >= 512 (several flips of random sign, each 2^-15 |s_k| |W_nk|) the fp32 allowance carries them.  PRO 0 and PRO 1 split rows that the
    emulation has bit for bit (x, and x - x0 with the kernel's x0): no such term."""
    assert t["kind"] == "pro2"
    return 2.0 ** -15 * pro2_rows(t, F64).abs().max(dim=1, keepdim=True).values * t["W"].double().abs().max(dim=1).values[None, :]


def check_emul(t, out, what=None, flip=False):
    """The pinning gate (flip: + front_flip(), for a KERNEL's PRO 2 output).  Returns the largest |out - emul| / allowance."""
    _, allow, _ = G.gate(t)
    rows, o = _rows_of(t, out)
    a = allow[rows].expand(len(rows), t["N"])
    if flip:
        a = a + front_flip(t)[rows]
    e = _emul_cached(t)[rows]
    G.assert_close_f32(o, e, a, what or f"{t.get('name', t['kind'])} (against the emulation)", frames=t.get("frames", 0), nb=t.get("nb", 0))
    return float(((o.double() - e).abs() / a.clamp_min(1e-300)).max())


def figures(t, out):
    """(max |out - ref64|, max |out - emul|, fp32 calibration, largest split term) over the valid rows, for printing"""
    ref, _, cal = G.gate(t)
    rows, o = _rows_of(t, out)
    o = o.double()
    return (float((o - ref[rows]).abs().max()), float((o - _emul_cached(t)[rows]).abs().max()), cal, float(split_term(t)[rows].max()))


def rejected(fn, t, out):
    try:
        fn(t, out)
    except AssertionError:
        return True
    return False


# ---- the Linears Denoiser<float> launches on the split loop --------------------------------------------------------------------------------
# Read off diffsheg_amd/csrc/denoiser.hip: every fp32 Linear of more than 512 rows goes through gemm() (:348-369, PRO 0) or gemm_pro()
# (:371-388, PRO 1 / 2), and pick_mma() (:286) hands both the packed weight under precision "bf16x3".  One row per FORM (N, K, front,
# activation, residual), for both configs (SHOW: C = 129 | 103, T = 88; BEAT: 141 | 51, T = 34) and the single-transformer model (SHOW, all
# 232 channels); D = 512, ff = 1024, time embedding 2 048, FiLM table 8 layers x 4 D = 16 384, encoder_aud D = 128.  The row's `where` names
# the call.  The activation codes are the launch's: 0 none, 1 SiLU, 2 GELU.  The funnel takes a Linear only with a bias, N % 4 == 0, no
# periodic residual and no activation behind the residual: joint_embed (positional residual, :1055 / :1059), time_embed.2 of the motion
# encoders (SiLU behind the speaker term, :1018), the `out` heads of 129 / 103 / 141 / 51 columns and encoder_aud's last Linear (two outputs,
# :1228) stay on the tiled GEMM and have no row here.  conv2 (K = 384) has no bias today, so the funnel passes it by as well; its form is
# kept in the table - it is the only K that is a multiple of 32 and not of 64 besides the grid's 32 and 96, and a bias would put it on
# this loop unnoticed.
FILM_LAST = 7 * 4 * 512                       # FiLM offset of layer 7's attention-branch StylizationBlock (run_encoder: l * 4 * D)
MODEL_LINEARS = {
    # ---- set_condition: the HuBERT-feature conv pair as GEMMs over im2col rows
    "conv1":          ("denoiser.hip:931 gemm(E->conv1), K = 3 x 1 024", lambda M: G.pro0_inputs(M, 128, 3072, act=2, res=False)),
    "conv2":          ("denoiser.hip:934 / :936 gemm(E->conv2), K = 3 x 128", lambda M: G.pro0_inputs(M, 128, 384, act=0, res=False)),
    # ---- the embedding Linears, on the batch's clips (above 512 clips)
    "time_embed.0":   ("denoiser.hip:1017 / :1197 gemm(te0)", lambda M: G.pro0_inputs(M, 2048, 512, act=1, res=False)),
    "aud_time_embed.2": ("denoiser.hip:1198 gemm(aud_te2)", lambda M: G.pro0_inputs(M, 2048, 2048, act=1, res=False)),
    "pid_embed.2":    ("denoiser.hip:912 gemm(E->pe2)", lambda M: G.pro0_inputs(M, 2048, 2048, act=0, res=False)),
    "film":           ("denoiser.hip:1019 gemm(E.film): the stacked FiLM Linears", lambda M: dict(G.pro0_inputs(M, 16384, 2048, act=0, res=False), cal_cols=torch.arange(0, 16384, 16))),
    "aud_film":       ("denoiser.hip:1199 gemm(aud_film)", lambda M: G.pro0_inputs(M, 512, 2048, act=0, res=False)),
    # ---- per evaluation, on the conditional rows
    "audio_proj":     ("denoiser.hip:1025 / :1028 gemm(E.aproj), [mel | aud_feat]", lambda M: G.pro0_inputs(M, 256, 256, act=0, res=False)),
    "audio_proj-single": ("denoiser.hip:1028 gemm(E.aproj), the mel features alone", lambda M: G.pro0_inputs(M, 256, 128, act=0, res=False)),
    "feat_proj.1-show-ges": ("denoiser.hip:1087 gemm_pro(L.f1, 1): h | audio_proj | hubert | 103 of 128", lambda M: G.pro1_inputs(M, 1024, (512, 256, 128, 128), 999, act=1, ld_extra=0)),
    "feat_proj.1-beat-ges": ("denoiser.hip:1087 gemm_pro(L.f1, 1): h | audio_proj | hubert | 51 of 64", lambda M: G.pro1_inputs(M, 1024, (512, 256, 128, 64), 947, act=1, ld_extra=0)),
    "feat_proj.1-exp": ("denoiser.hip:1087 gemm_pro(L.f1, 1): three segments", lambda M: G.pro1_inputs(M, 1024, (512, 256, 128, 0), 896, act=1, ld_extra=0)),
    "feat_proj.1-off-200": ("denoiser.hip:1087, rows at offset -200 (the PRO 1 shift)", lambda M: G.pro1_inputs(M, 1024, (512, 256, 128, 128), 999, act=1, ld_extra=0, family="off-200")),
    "feat_proj.3":    ("denoiser.hip:1088 gemm(L.f3), in-place residual", lambda M: G.pro0_inputs(M, 512, 1024, act=0, res=True, alias=True)),
    # ---- per evaluation, on both CFG halves
    "qkv-folded":     ("denoiser.hip:982 gemm_pro(L.qkv, 1)", lambda M: G.pro1_inputs(M, 1536, (512, 0, 0, 0), 512, act=0, ld_extra=0)),
    "qkv":            ("denoiser.hip:978 / :981 gemm(L.qkv)", lambda M: G.pro0_inputs(M, 1536, 512, act=0, res=False)),
    "sty1.out-show":  ("denoiser.hip:995 gemm_pro(L.sty1.out, 2), T = 88, last layer's FiLM offset", lambda M: G.pro2_inputs(M, 512, 512, 88, 6, film_off=FILM_LAST)),
    "sty1.out-beat":  ("denoiser.hip:993 gemm(L.sty1.out), front in the attention launch", lambda M: G.pro0_inputs(M, 512, 512, act=0, res=True, alias=True)),
    "ffn.linear1":    ("denoiser.hip:1000 gemm(L.ffn1)", lambda M: G.pro0_inputs(M, 1024, 512, act=2, res=False)),
    "ffn.linear2":    ("denoiser.hip:1001 gemm(L.ffn2)", lambda M: G.pro0_inputs(M, 512, 1024, act=0, res=False)),
    "sty2.out-beat":  ("denoiser.hip:1002 gemm_pro(L.sty2.out, 2), T = 34, FiLM offset + 2 D", lambda M: G.pro2_inputs(M, 512, 512, 34, 19, film_off=FILM_LAST + 1024)),
    "out-single":     ("denoiser.hip:1179 gemm(E.out): 232 columns (the heads of 129 / 103 / 141 / 51 are not multiples of 4)", lambda M: G.pro0_inputs(M, 232, 512, act=0, res=False)),
    # ---- encoder_aud (D = 128), on the conditional rows
    "aud.qkv":        ("denoiser.hip:505 gemm(aud.qkv)", lambda M: G.pro0_inputs(M, 384, 128, act=0, res=False)),
    "aud.sty1.out":   ("denoiser.hip:958 gemm(L.sty1.out), residual from another buffer", lambda M: G.pro0_inputs(M, 128, 128, act=0, res=True, alias=False)),
    "aud.ffn.linear1": ("denoiser.hip:959 gemm(L.ffn1)", lambda M: G.pro0_inputs(M, 1024, 128, act=2, res=False)),
    "aud.ffn.linear2": ("denoiser.hip:960 gemm(L.ffn2)", lambda M: G.pro0_inputs(M, 128, 1024, act=0, res=False)),
}
MODEL_M = (513, 641)        # the smallest row count on the split loop (f32_min_rows + 1), and one that straddles the 128-row tile edge at 640


def model_case(name, M):
    t = MODEL_LINEARS[name][1](M)
    t["name"] = f"split-model-{name}-M{M}"
    return t


# ---- the family cases of the CPU test (K = 512, and 960 with 13 padded columns for PRO 1) ------------------------------------------------
def family_case(pro, family, K):
    if pro == 0:
        t = G.pro0_inputs(200, 128, K, act=0, res=True, family=family)
    elif pro == 1:
        t = G.pro1_inputs(200, 192, G.FAMILY_WIDTHS, 947, act=1, family=family) if K == 960 else G.pro1_inputs(200, 128, (K, 0, 0, 0), K, family=family)
    else:
        t = G.pro2_inputs(200, 128, K, 34, 3, family=family)
    t["name"] = f"split-p{pro}-{family}-{K}"
    return t
