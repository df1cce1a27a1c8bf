"""Gates for the bf16 kernel tests, derived from the arithmetic and never from a kernel's output (plain torch, CPU).

A bf16 kernel that accumulates exact bf16 products in fp32 and stores the result rounded to nearest even can differ from the fp64
value of the same expression by at most
    half a bf16 ulp of the result  (the store)
  + K * 2^-23 * sum_k |x_k w_k|    (accum_bound: worst case of an fp32 accumulation in ANY order; 2^-23 rather than 2^-24 because the
                                    matrix pipe need not round to nearest internally).
assert_rounded / assert_close_f32 check exactly that on EVERY element and name the worst one with its position inside the 32 x 32
tile, its clip and its frame, so that a routing fault locates itself.

Chains with an internal bf16 rounding point (LayerNorm + FiLM + SiLU prologue, the FFN's hidden and SiLU outputs, the MFMA attention
kernels' k^ / A / q^) cannot be bounded that way: a value that sits on a rounding boundary flips with the last bit of the arithmetic in front
of it, and one flip moves the output by ulp(operand) * |w|.  Their slack is CALIBRATED on the CPU: the chain is evaluated in fp64 and
in fp32 with the same documented rounding points (and the documented 1e-4 approximation of the fast GELU as a uniform perturbation;
the kernel's polynomial is not copied), and
    slack    = MARGIN * max |fp32 chain - fp64 chain|          (one number per test, applied to every element)
    rms gate = MARGIN * rms (fp32 chain - fp64 chain) + rms of the output rounding.
MARGIN = 3: both differences are maxima of the same distribution of rounding flips; the kernel additionally carries the error of the
hardware exp / rcp and its own order of the LayerNorm statistics.

Where ONE rounded operand feeds the Linear directly (LayerNorm [+ FiLM + SiLU] prologue -> Linear) the realised maximum is a lottery:
an operand row of 512 values sees ~0.1 .. 1 flips, and the maximum over the test is decided by whether one of the few elements with
|s| >= 2 (ulp 2^-6, against 2^-9 for the typical element) is among them - the kernel and the CPU chain flip different elements, and on
an MI355X the kernel's maximum was 1.0 .. 924 x the calibration at the five (T, batch) shapes of the op test (the table below).  Those chains therefore
add flip_bound: the effect of one flip of the row's coarsest operand on the output's largest weight, max_k ulp(s_mk) * max_k |w_nk|
(2.7e-3 at these operands; a dropped k-term is 4e-2 .. 4e-1).  It is computed from the fp64 operands, not from any kernel output.

Observed on an MI355X, kernel / calibration (maximum of |out - fp64 chain|, the bf16 store's own half ulp taken off, over the maximum of
|fp32 chain - fp64 chain|); the gates allow MARGIN = 3, plus flip_bound where noted:
  fused FFN (v3-hilo, v3, v2)             300 rows: max 1.06, rms 1.02        1000 rows: max 1.47, rms 1.04
  bf16 attention (nb, T)                  (5, 88) 0.19   (3, 34) 0.04   (2, 96) 0.86   (4, 11) 0.00   (2, 30) 0.46
  LN + FiLM + SiLU -> Linear (pro 2),     (1000 rows, T 88, 7 clips) 1.73   (1000, 30, 6) 3.55   (1000, 34, 5) 1.00
    both generations, fp32 and hi / lo    (300, 64, 3) 226 and (44, 11, 4) 924: the CPU chain has no flip at all in these rows (calibration
                                          8.1e-7 / 6.9e-7), the kernel one of 1.8e-4 / 6.3e-4 - at most 0.68 of flip_bound, which carries
                                          these chains (the kernel's maximum is 2.0e-3 .. 2.3e-3 at the 1000-row shapes)
  LN -> Linear, normalise-first (pro 1,   (1000, 88, 7) 3.89   (300, 64, 3) 3.41 - its statistics are E[x^2] - mean^2 of fp32 sums, more
    first generation)                     flips than torch's LayerNorm; with flip_bound the worst element uses 0.84 of its allowance
  fused encoder_aud tail (Mc, T, nb),     (300, 88, 4) 0.64 / 1.02   (44, 11, 4) 1.31 / 1.13   (290, 34, 9) 1.06 / 1.01   (300, 88, 1) 0.95 / 1.02
    max / rms, + flip_bound               (257, 88, 3) 1.05 / 0.95   (513, 30, 6) 1.11 / 1.06; kernel maximum 5.8e-3 .. 9.1e-3, flip_bound <= 1.2e-2
                                          offset on b2 (300, 88, 4): rms error 8.0e-4 (0), 8.4e-4 (+20), 1.7e-3 (-100); ln_raw_moment_slack allows far
                                          more at -100 (1.3 at the worst element: its bound is the worst case of 128 fp32 additions)
  attention, per kernel form              worst element / allowance (0.5 ulp of a bf16 store + 3 x calibration [+ attn_flip_slack]), the largest over the six input
    (test_gpu_bf16_attention_families.py, families, dense / ragged / CFG-doubled, and the family and shape that produced it:
     bf16_gates.ATTN_FORMS)               tiled MFMA      0.999 plain, T 11, 3 clips dense (the store's half ulp; calibration 1.1e-6); WITHOUT attn_flip_slack 10.2 (v_small, T 11)
                                          row-major MFMA  0.999 plain, T 11, 3 clips dense; without attn_flip_slack 1.86 (plain, T 88, dense)
                                          tiled, two halves and rev (dsh_op_linear_attention_tiled)  0.999 plain, T 34, 3 + 3 clips ragged; without 2.04 (v_small, T 88)
                                          pre-loaded VALU bf16 0.999 v_small, D 128, T 11 dense     fp32 0.417 v_out, D 128, T 96, 7 clips ragged (kernel / calibration 1.25)
                                          loop VALU       bf16 0.999 plain, D 128, T 97 dense       fp32 0.667 k_tie, D 128, T 120, 7 clips ragged (kernel / calibration 2.0)
                                          Derived term: attn_flip_slack, MFMA forms only.  Without it 9 of the 48 dense MFMA cases failed, each in 1 .. 12 elements fed by
                                          an operand that the fp64 chain puts on a bf16 rounding tie - e.g. k^ = 0.22314 of frame 8, channel
                                          23, head 2, clip 2 at T 11, 1.9e-8 (relative) from the tie: the tiled kernel rounds it to the other neighbour than the row-major kernel and both CPU chains, and
                                          ulp(k^) |v| = 3.3e-3 then moves A[23][29] = 9.1e-3 by 54 of its ulps.  The VALU forms needed no term.
Every mutant of test_bf16_gates_cpu.py is rejected with these gates.

The input builders below restate the generator sequences of the op tests in test_gpu_ops.py, so that test_bf16_gates_cpu.py checks the
gates on the very operands the GPU tests use.
"""
import torch
import torch.nn.functional as F

MARGIN = 3.0
GELU_APPROX = 1e-4          # tl_common.h documents 9.5e-5 for gelu_fast against the erf form
_ACTS = {0: lambda v: v, 1: F.silu, 2: F.gelu}


# ---- elementary gates ----------------------------------------------------------------------------------------------------------------
def ulp_bf16(v):
    """2^(floor(log2 |v|) - 7) in fp64; |v| below the smallest normal (2^-126, 0 included) takes the denormal spacing 2^-133."""
    a = torch.as_tensor(v, dtype=torch.float64).abs()
    _, e = torch.frexp(a.clamp_min(2.0 ** -126))              # a = m 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    return torch.ldexp(torch.ones_like(a), e - 8)


def accum_bound(absx, absw, K):
    """K * 2^-23 * (|X| @ |W|^T): worst-case error of accumulating the K exact products of a row in fp32, in any order."""
    return K * 2.0 ** -23 * (absx.double().abs() @ absw.double().abs().T)


def _locate(err, allow, frames, nb):
    excess = err - allow
    excess = torch.where(torch.isnan(excess), torch.full_like(excess, float("inf")), excess)
    i = int(excess.argmax())
    ncol = err.shape[-1]
    r, c = i // ncol, i % ncol
    msg = f"worst element row {r} col {c} (row % 32 = {r % 32}, col % 32 = {c % 32}"
    if frames:
        msg += f", clip {(r // frames) % max(nb, 1)}, frame {r % frames}"
    return r, c, msg + ")"


def _check(out, ref64, allow, what, frames, nb):
    o = out.detach().cpu().double().reshape(-1, out.shape[-1])
    ref = ref64.detach().cpu().double().reshape(o.shape)
    allow = allow.reshape(o.shape) if allow.dim() else allow.expand(o.shape)
    err = (o - ref).abs()
    bad = ~(err <= allow)                                      # NaN / Inf in the output fail
    if bool(bad.any()):
        r, c, where = _locate(err, allow, frames, nb)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the gate; {where}: out {float(o[r, c])!r} "
                             f"ref {float(ref[r, c])!r} |diff| {float(err[r, c]):.3e} allowed {float(allow[r, c]):.3e}")
    return float((err / allow.clamp_min(1e-300)).max())


def assert_rounded(out_bf16, ref64, slack=0.0, what="bf16 output", frames=0, nb=0):
    """Every element: |out - ref| <= 0.5 ulp_bf16(max(|out|, |ref|)) + slack.  Returns the largest |diff| / allowance."""
    o = out_bf16.detach().cpu().double()
    r = ref64.detach().cpu().double().reshape(o.shape)
    big = torch.maximum(o.abs(), r.abs())
    big = torch.where(torch.isfinite(big), big, torch.zeros_like(big))
    allow = 0.5 * ulp_bf16(big) + torch.as_tensor(slack, dtype=torch.float64)
    return _check(out_bf16, ref64, allow.reshape(-1, o.shape[-1]), what, frames, nb)


def assert_close_f32(out_f32, ref64, slack, what="fp32 output", frames=0, nb=0):
    """Every element: |out - ref| <= slack (the fp32 store itself is inside accum_bound for every K >= 2)."""
    o = out_f32.detach().cpu().double()
    allow = torch.as_tensor(slack, dtype=torch.float64)
    if allow.dim():
        allow = allow.reshape(-1, o.shape[-1])
    return _check(out_f32, ref64, allow, what, frames, nb)


def assert_rms(out, ref64, gate, what="rms"):
    rms = float((out.detach().cpu().double() - ref64.double()).pow(2).mean().sqrt())
    assert rms <= gate, f"{what}: rms error {rms:.3e} above the gate {gate:.3e}"
    return rms / gate


def bf16_rounding_rms(ref64):
    """rms of the round-to-nearest bf16 store of ref: ulp / sqrt(12) per element."""
    return float((ulp_bf16(ref64) ** 2 / 12.0).mean().sqrt())


def calibrate(chain32, chain64, margin=MARGIN):
    """(slack, rms gate without output rounding) of a chain with internal bf16 rounding points: margin * (max, rms) of the difference
    between its fp32 and its fp64 evaluation."""
    d = chain32.double() - chain64.double()
    return margin * float(d.abs().max()), margin * float(d.pow(2).mean().sqrt())


def flip_bound(s, W):
    """One rounding flip of the coarsest bf16 operand of row m, met by the largest weight of output n: max_k ulp(s_mk) * max_k |w_nk|."""
    return ulp_bf16(s).max(dim=1, keepdim=True).values * W.double().abs().max(dim=1).values[None, :]


def prologue_slack(t, Mv, T, nb, pro, act, ref64, **kw):
    """Slack of a LayerNorm [+ FiLM + SiLU] -> bf16 -> Linear chain: MARGIN x calibration + one worst-placed flip.  Returns (slack, cal)."""
    cal = float((tl_chain(t, Mv, T, nb, pro, act, torch.float32, **kw).double() - ref64).abs().max())
    return MARGIN * cal + flip_bound(tl_prologue(t, Mv, T, nb, pro, torch.float64, **kw), t["W"]), cal


SILU_LIP = 1.1             # max |d silu / dx| = 1.0998: a pre-activation slack s becomes SILU_LIP * s behind a SiLU (GELU: 1.13)
GELU_LIP = 1.13


def silu_hw(y):
    """Allowance for the hardware exp and rcp of a SiLU epilogue: 2^-18 |y| (two ~1 ulp fp32 transcendentals and the multiply, with
    room; assumed, not measured - the exact-operand tests record the observed maximum)."""
    return 2.0 ** -18 * y.double().abs()


def hilo_slack(R, ref):
    """Residual stream as hi / lo bf16 planes (tl_common.h): lo = bf16(h - hi) leaves <= 2^-17 relative per store - once when the op
    splits R, once when the kernel splits its fp32 result."""
    return 2.0 ** -17 * (R.double().abs() + ref.double().abs())


def rne(x, dt):
    return x.bfloat16().to(dt)


def truncate_bf16(x):
    """fp -> bf16 by dropping the low 16 bits of the fp32 pattern (the store mutant)."""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()


# ---- token-per-lane Linear (test_tl_linear_all_denoiser_variants) -------------------------------------------------------------------
def tl_inputs(K, N, pro, res, Mv, T, nb):
    """The operands of test_tl_linear_all_denoiser_variants (same generator, same order), on the CPU."""
    M = (Mv + 127) // 128 * 128
    g = torch.Generator().manual_seed(K + N + pro)
    t = {"X": (torch.randn(M, K, generator=g) * 1.5 + 0.3).bfloat16(), "W": (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16(),
         "b": torch.randn(N, generator=g)}
    t["R"] = torch.randn(M, N, generator=g) if res else None
    t["gam"] = 1 + 0.1 * torch.randn(K, generator=g)
    t["bet"] = 0.1 * torch.randn(K, generator=g)
    t["film"] = 0.3 * torch.randn(nb, 2 * K, generator=g)
    return t


def tl_prologue(t, Mv, T, nb, pro, dt, kreal=None, film_rows=None):
    """The bf16 operand rows the Linear multiplies: X itself (pro 0), or LayerNorm (pro 1 / 3) [+ FiLM + SiLU (pro 2)] rounded to bf16.
    film_rows: clip index per row (default (row // T) % nb)."""
    K = t["X"].shape[1]
    kreal = kreal or K
    x = t["X"][:Mv].to(dt)
    if pro == 0:
        return x
    xr = x[:, :kreal]
    y = F.layer_norm(xr, (kreal,), t["gam"][:kreal].to(dt), t["bet"][:kreal].to(dt), 1e-5)
    if pro == 2:
        rows = torch.arange(Mv)
        f = t["film"].to(dt)[(rows // T) % nb if film_rows is None else film_rows]
        y = F.silu(y * (1 + f[:, :K]) + f[:, K:])
    out = torch.zeros(Mv, K, dtype=dt)
    out[:, :kreal] = rne(y, dt)
    return out


def tl_chain(t, Mv, T, nb, pro, act, dt, kreal=None, reverse=False, gelu_noise=None, **kw):
    """prologue -> Linear -> activation -> + residual in dtype dt; reverse: the K order of the accumulation flipped."""
    xin = tl_prologue(t, Mv, T, nb, pro, dt, kreal, **kw)
    W = t["W"].to(dt)
    y = (xin.flip(1) @ W.flip(1).T if reverse else xin @ W.T) + t["b"].to(dt)
    y = _ACTS[act](y)
    if act == 2 and gelu_noise is not None:
        y = y + gelu_noise.to(dt)
    if t["R"] is not None:
        y = y + t["R"][:Mv].to(dt)
    return y


def gelu_noise(shape, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * GELU_APPROX


def tl_folded(t, Mv, pro, act, kreal=None):
    """The folded-LayerNorm Linear of the second generation, from the operands the production packer builds:
    W' = bf16(gamma * W), c = sum_k W', d = b + W beta, y = rstd (x W'^T - mean c) + d, in fp64; and the slack of its fp32 evaluation.
      * x W'^T: accum_bound, scaled by rstd;
      * mean (an fp32 sum of K values): K 2^-23 mean|x|, times rstd |c|, plus the fp32 rounding of c;
      * rstd: the variance is E[x^2] - mean^2 of fp32 sums, K 2^-23 (E[x^2] + mean^2) absolute, i.e. half of that over var relative
        on rstd, plus 2^-22 for the hardware rsq — times |y - d| (the cancellation term of the large-mean test:
        it grows with mean^2 / var);
      * four fp32 roundings of the epilogue on |rstd S|, |rstd mean c|, |d|.
    Returns (reference of the pre-activation, slack of the pre-activation, reference after the activation)."""
    K = t["X"].shape[1]
    kreal = kreal or K
    x = t["X"][:Mv].double()
    Wf = (t["W"].float() * t["gam"].float()).bfloat16().double()
    Wf[:, kreal:] = 0
    c = Wf.sum(1).float().double()
    d = (t["b"].double() + t["W"].double()[:, :kreal] @ t["bet"].double()[:kreal]).float().double()
    xr = x[:, :kreal]
    mean = xr.mean(-1, keepdim=True)
    ex2 = (xr * xr).mean(-1, keepdim=True)
    var = ex2 - mean * mean
    rstd = 1 / torch.sqrt(var + 1e-5)
    S = xr @ Wf[:, :kreal].T
    y = rstd * (S - mean * c) + d
    eps = 2.0 ** -23
    rel_rstd = 0.5 * K * eps * (ex2 + mean * mean) / var + 2 * eps
    slack = (rstd * (accum_bound(xr, Wf[:, :kreal], K) + c.abs() * (K * eps * xr.abs().mean(-1, keepdim=True) + eps * mean.abs()))
             + rel_rstd * (y - d).abs() + 4 * eps * (rstd * (S.abs() + (mean * c).abs()) + d.abs()))
    return y, slack, _ACTS[act](y)


# ---- fused FFN (test_tl2_ffn_fused_matches_reference) ---------------------------------------------------------------------------------
def ffn_inputs(Mv, T, nb, n_const):
    D, Fh = 512, 1024
    M = (Mv + 127) // 128 * 128
    g = torch.Generator().manual_seed(Mv + T)
    t = {"X": (torch.randn(M, D, generator=g) * 1.2 + 0.2).bfloat16(), "H": torch.randn(M, D, generator=g),
         "W1": (torch.randn(Fh, D, generator=g) / D ** 0.5).bfloat16(), "W2": (torch.randn(D, Fh, generator=g) / Fh ** 0.5).bfloat16(),
         "W3": (torch.randn(D, D, generator=g) / D ** 0.5).bfloat16()}
    t["b1"], t["b2"], t["b3"] = (0.3 * torch.randn(n, generator=g) for n in (Fh, D, D))
    t["gam"] = 1 + 0.1 * torch.randn(D, generator=g)
    t["bet"] = 0.1 * torch.randn(D, generator=g)
    t["film"] = 0.3 * torch.randn(nb, 2 * D, generator=g)
    t["rc"] = torch.randn(D, generator=g)
    return t


def ffn_chain(t, Mv, T, nb, n_const, dt, reverse=False, noise=None, film_rows=None, w3=None, b3=None):
    """linear1 -> GELU -> bf16 -> linear2 -> LayerNorm -> FiLM -> SiLU -> bf16 -> linear3 -> + H (+ row constant), in dtype dt."""
    D = 512
    mm = (lambda a, w: a.flip(1) @ w.flip(1).T) if reverse else (lambda a, w: a @ w.T)
    hid = F.gelu(mm(t["X"][:Mv].to(dt), t["W1"].to(dt)) + t["b1"].to(dt))
    if noise is not None:
        hid = hid + noise.to(dt)
    hid = rne(hid, dt)
    y2 = mm(hid, t["W2"].to(dt)) + t["b2"].to(dt)
    rows = torch.arange(Mv)
    f = t["film"].to(dt)[(rows // T) % nb if film_rows is None else film_rows]
    s_ = F.silu(F.layer_norm(y2, (D,), t["gam"].to(dt), t["bet"].to(dt), 1e-5) * (1 + f[:, :D]) + f[:, D:])
    W3 = t["W3"].to(dt) if w3 is None else w3.to(dt)
    bb = t["b3"].to(dt) if b3 is None else b3.to(dt)
    y = mm(rne(s_, dt), W3) + bb + t["H"][:Mv].to(dt)
    if n_const:
        y[:n_const] += t["rc"].to(dt)
    return y


# ---- linear attention: every bf16 kernel form of attention.hip and the fp32 instantiations of its VALU templates ------------------------
# Rounding points, read from attention.hip:
#   linear_attention_tiled_kernel, linear_attention_mfma_kernel (hd 64, <= 96 frames): exp, sums and 1 / sum in fp32; k^ = e * inv is rounded to
#     bf16 AFTER the normalisation (pack2_bf16 of the product), A = k^T v is accumulated in fp32 and rounded to bf16 as the operand of the second
#     product, q^ = e * inv is rounded to bf16, y is accumulated in fp32 and stored rounded to nearest: rounded=True.
#   linear_attention_pre_kernel, linear_attention_kernel (bf16 and fp32 storage, hd 16 and 64): to_f32 at the loads, everything in fp32 registers
#     and LDS (k^, A, q^ are never rounded), from_f32 (round to nearest even) at the store: rounded=False.  One accumulator per output, frames
#     (A) and channels (y) ascending: seq=True evaluates the fp32 chain in that class of order, and its reverse.
ATTN_FAMILIES = ("plain", "v_out", "v_small", "k_sat", "q_sat", "k_tie")
# form -> (dtype argument of dsh_op_linear_attention_ragged, variant, the kernel rounds k^ / A / q^ to bf16, ((D, hd, T), ...)): the smallest
# shapes at which each form changes behaviour (one frame block of 12, 32-frame groups of q, the 96-frame limit and the first length above it)
ATTN_FORMS = {
    "tiled": (1, 0, True, tuple((512, 64, T) for T in (11, 33, 88, 96))),
    "mfma": (1, 1, True, tuple((512, 64, T) for T in (11, 33, 88, 96))),
    "pre_bf16": (1, 1, False, tuple((128, 16, T) for T in (11, 34, 96))),
    "pre_f32": (0, 0, False, tuple((128, 16, T) for T in (11, 34, 96))),
    "loop_bf16": (1, 1, False, ((128, 16, 97), (128, 16, 120), (512, 64, 97), (512, 64, 120))),
    "loop_f32": (0, 0, False, ((128, 16, 97), (128, 16, 120), (512, 64, 97), (512, 64, 120))),
}
ATTN_ROWS = [(form, D, hd, T) for form, (_, _, _, shapes) in ATTN_FORMS.items() for D, hd, T in shapes]
ATTN_NB = 3                 # dense batches: odd, so the tiled helper's two halves are 2 and 1 clips


def attn_lens(T):
    """Lengths of a ragged batch padded to T frames: one frame, the edges of the kernels' frame blocks (12 k, 32, 33), T - 1 and T."""
    return sorted({1, 12, 24, 32, 33, T - 1, T} & set(range(1, T + 1)))


def attn_inputs(nb, T, family="plain", D=512, hd=64):
    """qkv [nb, T, 3 D] in bf16.  The families are applied before the rounding; "plain" at D = 512 is the recipe of
    test_linear_attention_bf16_mfma, generator sequence included."""
    g = torch.Generator().manual_seed(T + nb + (512 - D))
    x = torch.randn(nb, T, 3 * D, generator=g) * 2
    if family == "v_out":                     # A = sum k^ v = 300 sum k^ in that column: the normalisation against k^'s rounding point
        x[:, :, 2 * D + 7] = 300.0
    elif family == "v_small":                 # gates that scale with a clamped range; flushing
        x[:, :, 2 * D:] *= 1e-3
    elif family == "k_sat":                   # max-subtraction, exp(-40), weights of exactly 1 and 0
        x[:, T // 2, D:2 * D] += 40.0
    elif family == "q_sat":                   # the same for the channel softmax
        x[:, :, :D].view(nb, T, D // hd, hd)[..., 3] += 30.0
    elif family == "k_tie":                   # weights of 1 / n, which bf16 cannot represent; a wrong frame count
        x[:, :, D:2 * D] = x[:, :1, D:2 * D]
    elif family != "plain":
        raise ValueError(family)
    return x.bfloat16()


def attn_chain(qkv, dt, lens=None, hd=64, rounded=True, reverse=False, seq=False, frames_delta=0, k_round_early=False, q_group=None, fast_exp=False):
    """y = softmax_channels(q) (softmax_time(k)^T v) per head, [nb, T, D] in dtype dt.
    rounded: the values rounded to bf16 on the way - True = ("k", "A", "q") as the MFMA kernels do, False = none (the VALU templates), or a
             tuple of those names (the mutants of the VALU forms).
    lens:    frames per clip that enter the time-softmax, clip b takes lens[b % len(lens)] (rows behind them are excluded by selection;
             every one of the T query rows is answered).  A list of nb entries gives every clip its own length (the lens[b] mutant).
    reverse: the order of every accumulation flipped (frames in the time-softmax and in A, channels in y).
    seq:     fp32 only: one accumulator per output, the terms added one at a time (sum of the exponentials, A over the frames, y over the
             head's channels) - the class of order of the VALU kernels; otherwise torch's softmax and einsum.
    fast_exp: both softmaxes as e = exp2(x log2e - max log2e), e * (1 / sum e) in dt - the MFMA kernels' documented evaluation (their
             v_exp_f32 itself is not copied): an fp32 chain whose roundings fall elsewhere than torch's, for the CPU proof of attn_flip_slack.
    Mutants: frames_delta = +1 / -1: one frame more / fewer in the time-softmax and in A (never fewer than one; the frame behind a full
             window is the clamped load every kernel issues, a duplicate of frame T - 1);  k_round_early: e = exp(k - max) rounded to bf16,
             the normalisation applied behind the rounding;  q_group: the channel softmax taken over groups of that many channels."""
    nb, T, D3 = qkv.shape
    D = D3 // 3
    H = D // hd
    pts = ("k", "A", "q") if rounded is True else tuple(rounded or ())
    r = lambda name, v: rne(v, dt) if name in pts else v
    seq = seq and dt == torch.float32
    out = torch.zeros(nb, T, D, dtype=dt)
    for b in range(nb):
        n = max(1, (T if lens is None else int(lens[b % len(lens)])) + frames_delta)
        q, k, v = (qkv[b, :, i * D:(i + 1) * D].to(dt).view(T, H, hd) for i in range(3))
        if n > T:
            k, v = torch.cat((k, k[T - 1:]), 0), torch.cat((v, v[T - 1:]), 0)
        k, v = k[:n], v[:n]
        if reverse:
            k, v = k.flip(0), v.flip(0)
        if fast_exp:
            L = torch.tensor(1.44269504088896341, dtype=dt)
            sm = lambda x, dim: (lambda e: e * (1 / e.sum(dim=dim, keepdim=True)))(torch.exp2(x * L + (-x.max(dim=dim, keepdim=True).values * L)))
            kh, qh = r("k", sm(k, 0)), r("q", sm(q, -1))
        elif k_round_early or seq:
            e = (k - k.max(dim=0).values).exp()
            ssum = e.sum(0)
            if seq:
                ssum = torch.zeros(H, hd)
                for t in range(n):
                    ssum += e[t]
            kh = rne(e, dt) / ssum if k_round_early else r("k", e * (1 / ssum))
        else:
            kh = r("k", k.softmax(dim=0))
        if not fast_exp:
            qh = r("q", q.reshape(T, D // (q_group or hd), q_group or hd).softmax(dim=-1).view(T, H, hd))
        if seq:
            A = torch.zeros(H, hd, hd)
            for t in range(n):
                A.addcmul_(kh[t][:, :, None], v[t][:, None, :])
            A = r("A", A)
            y = torch.zeros(T, H, hd)
            for d in (range(hd - 1, -1, -1) if reverse else range(hd)):
                y.addcmul_(qh[:, :, d, None], A[None, :, d, :])
        else:
            A = r("A", torch.einsum("nhd,nhl->hdl", kh, v))
            y = torch.einsum("nhd,hdl->nhl", qh.flip(2), A.flip(1)) if reverse else torch.einsum("nhd,hdl->nhl", qh, A)
        out[b] = y.reshape(T, D)
    return out


def attn_valid(nb, T, lens=None):
    """[nb, T] bool: the query rows whose value is specified (frames inside the clip's length)."""
    n = torch.tensor([T if lens is None else int(lens[b % len(lens)]) for b in range(nb)])
    return torch.arange(T)[None, :] < n[:, None]


def attn_gate(qkv, hd, rounds, lens=None):
    """(fp64 chain, calibration, flip allowance) of one kernel form on these operands: calibration = max |fp32 chain - fp64 chain| over the
    valid rows; for the VALU forms (rounds = False) the maximum over both orders of the one-accumulator fp32 chain, as f32_gates.gate takes
    it.  The gate of every form and family is assert_rounded / assert_close_f32 with slack MARGIN x calibration, plus, for the MFMA forms,
    attn_flip_slack (an [nb, T, D] tensor; 0.0 for the VALU forms, whose only rounding is the store)."""
    kw = dict(lens=lens, hd=hd, rounded=rounds)
    ref = attn_chain(qkv, torch.float64, **kw)
    valid = attn_valid(qkv.shape[0], qkv.shape[1], lens)
    cal = max(float((attn_chain(qkv, torch.float32, reverse=rev, seq=not rounds, **kw).double() - ref)[valid].abs().max())
              for rev in ((False,) if rounds else (False, True)))
    return ref, cal, (attn_flip_slack(qkv, hd, lens) if rounds else 0.0)


def _tie_distance(x):
    """distance of |x| from the nearest midpoint between two neighbouring bf16 values (where round-to-nearest changes its mind)"""
    u = ulp_bf16(x)
    return ((x.abs() / u) % 1.0 - 0.5).abs() * u


def attn_flip_slack(qkv, hd=64, lens=None):
    """What the MFMA kernels' fast exponentials may cost, per output element [nb, T, D], from the fp64 operands alone.
    The kernels evaluate e = exp(x - m) as v_exp_f32(x log2e - m log2e) (tiled: one fma on a rounded -m log2e; row-major: __expf, the rounded
    product (x - m) log2e).  v_exp_f32 is documented to 1 ulp; the argument carries 2^-24 (|x - m| + |m|) log2e absolute plus 2^-25 |x - m| log2e
    for the constant, i.e. on e a relative  rel_e <= 2^-24 (1.5 |x - m| + |m| + 2)  - torch's exp, which the calibration chain uses, is good to
    half an ulp at every argument.  A softmax weight of N terms then carries  eps = rel_e + sum_i p_i rel_e_i + (N + 2) 2^-24  (its own
    exponential, the sum's, the N fp32 additions, the reciprocal and the product).  That is far below a bf16 ulp, so it shows ONLY where the
    exact value lies within eps of a rounding tie: there the kernel may round k^ or q^ to the other neighbour (one ulp of the operand).  A
    flipped k^ moves A = sum_t k^ v by ulp(k^) |v| in front of A's own rounding; together with the accum_bound of the n fp32 products that
    decides whether A can round the other way, so the rounded A moves by at most  flip(A) = sum_t flip(k^) |v| + one ulp of A where it can
    round either way  (ulp(k^) |v| exceeds an ulp of A where A is small beside its terms).  The allowance of y[t, l] is the sum over the
    head's channels d of
        q^[t, d] flip(A[d, l]) + flip(q^[t, d]) (|A[d, l]| + flip(A[d, l])),    flip(k^ or q^) = its ulp_bf16 where it can round either way, else 0.
    It is exactly 0 for an output none of whose operands sits on a tie (most of them)."""
    nb, T, D3 = qkv.shape
    D = D3 // 3
    H = D // hd
    u = 2.0 ** -24

    def soft(x, dim, N):
        m = x.max(dim=dim, keepdim=True).values
        a = x - m
        p = a.exp()
        p = p / p.sum(dim=dim, keepdim=True)
        rel_e = u * (1.5 * a.abs() + m.abs() + 2)
        eps = rel_e + (p * rel_e).sum(dim=dim, keepdim=True) + (N + 2) * u
        return p, torch.where(_tie_distance(p) <= eps * p, ulp_bf16(p), torch.zeros_like(p))

    out = torch.zeros(nb, T, D, dtype=torch.float64)
    for b in range(nb):
        n = T if lens is None else int(lens[b % len(lens)])
        q, k, v = (qkv[b, :, i * D:(i + 1) * D].double().view(T, H, hd) for i in range(3))
        k, v = k[:n], v[:n]
        kh, fk = soft(k, 0, n)
        qh, fq = soft(q, -1, hd)
        khr, qhr = rne(kh, torch.float64), rne(qh, torch.float64)
        A = torch.einsum("nhd,nhl->hdl", khr, v)
        moved = torch.einsum("nhd,nhl->hdl", fk, v.abs())
        pert = moved + n * 2.0 ** -23 * torch.einsum("nhd,nhl->hdl", khr, v.abs())
        fA = moved + torch.where(_tie_distance(A) <= pert, ulp_bf16(A), torch.zeros_like(A))
        out[b] = (torch.einsum("nhd,hdl->nhl", qhr, fA) + torch.einsum("nhd,hdl->nhl", fq, rne(A, torch.float64).abs() + fA)).reshape(T, D)
    return out


def attn_ratio(out, ref, cal, T, lens=None, extra=0.0):
    """Largest |out - ref| / allowance over the valid rows, without asserting (printed in front of the assertion; NaN counts as inf)."""
    o, r = out.detach().cpu().double(), ref.double()
    allow = torch.full_like(r, MARGIN * cal) + extra
    if out.dtype == torch.bfloat16:
        big = torch.maximum(o.abs(), r.abs())
        allow = allow + 0.5 * ulp_bf16(torch.where(torch.isfinite(big), big, torch.zeros_like(big)))
    x = (o - r).abs() / allow.clamp_min(1e-300)
    x = torch.where(torch.isnan(x), torch.full_like(x, float("inf")), x)[attn_valid(o.shape[0], T, lens)]
    return float(x.max())


def attn_check(out, ref, cal, T, lens=None, what="attention", extra=0.0):
    """The valid rows of a bf16 (assert_rounded) or fp32 (assert_close_f32) output [nb, T, D] against the fp64 chain, slack MARGIN x
    calibration + extra (a number or [nb, T, D]), clip by clip so that the report names the clip and the frame; returns the largest
    |diff| / allowance."""
    nb, D = out.shape[0], out.shape[-1]
    fn = assert_rounded if out.dtype == torch.bfloat16 else assert_close_f32
    worst = 0.0
    for b in range(nb):
        n = T if lens is None else int(lens[b % len(lens)])
        slack = MARGIN * cal + (extra[b, :n].reshape(-1, D) if torch.is_tensor(extra) else extra)
        worst = max(worst, fn(out[b, :n].reshape(-1, D), ref[b, :n].reshape(-1, D), slack, f"{what}, clip {b} of {nb} ({n} frames)", frames=n, nb=1))
    return worst


def attn_wrong_half_lens(lens):
    """The lens[b] mutant of a CFG-doubled batch: the second half reads what lies behind the n_lens lengths (here: the lengths rotated by one)."""
    return list(lens) + list(lens[1:]) + list(lens[:1])


# ---- fused encoder_aud tail (tl_aud_tail_kernel, D = 128) -----------------------------------------------------------------------------
def aud_inputs(Mc, T, nb):
    """The operand recipe of ffn_inputs at D = 128.  The weights are fp32 tensors that hold bf16 values: dsh_op_tl_aud_tail takes the
    layer's fp32 weights and its packer rounds them, which is exact here."""
    D, Fh = 128, 1024
    g = torch.Generator().manual_seed(Mc + T)
    bw = lambda n, k: (torch.randn(n, k, generator=g) / k ** 0.5).bfloat16().float()
    t = {"Y": (torch.randn(Mc, D, generator=g) * 1.2 + 0.2).bfloat16(), "X2": torch.randn(Mc, D, generator=g),
         "Ws1": bw(D, D), "W1": bw(Fh, D), "W2": bw(D, Fh), "Ws2": bw(D, D)}
    t["bs1"], t["b1"], t["b2"], t["bs2"] = (0.3 * torch.randn(n, generator=g) for n in (D, Fh, D, D))
    for i in (1, 2):
        t[f"g{i}"] = 1 + 0.1 * torch.randn(D, generator=g)
        t[f"be{i}"] = 0.1 * torch.randn(D, generator=g)
    t["film"] = 0.3 * torch.randn(nb, 4 * D, generator=g)          # [scale1 | shift1 | scale2 | shift2]
    return t


def aud_stages(t, Mc, T, nb, dt, reverse=False, noise=None, film_rows=None, final_res="h"):
    """encoder_aud behind its attention with the rounding points tl_aud.hip documents: s1, bf16(h), the GELU output and s2 are rounded to
    bf16; LayerNorm 2 is taken from the fp32 y2; h stays in fp32 as the residual of the last Linear.  Returns every stage."""
    D = 128
    mm = (lambda a, w: a.flip(1) @ w.flip(1).T) if reverse else (lambda a, w: a @ w.T)
    rows = torch.arange(Mc)
    f = t["film"].to(dt)[(rows // T) % nb if film_rows is None else film_rows]
    sty = lambda v, i: F.silu(F.layer_norm(v, (D,), t[f"g{i}"].to(dt), t[f"be{i}"].to(dt), 1e-5) * (1 + f[:, 2 * (i - 1) * D:(2 * i - 1) * D])
                              + f[:, (2 * i - 1) * D:2 * i * D])
    x = t["X2"][:Mc].to(dt)
    s1 = rne(sty(t["Y"][:Mc].to(dt), 1), dt)
    h = x + (mm(s1, t["Ws1"].to(dt)) + t["bs1"].to(dt))
    hid = F.gelu(mm(rne(h, dt), t["W1"].to(dt)) + t["b1"].to(dt))
    if noise is not None:
        hid = hid + noise.to(dt)
    y2 = mm(rne(hid, dt), t["W2"].to(dt)) + t["b2"].to(dt)
    s2 = rne(sty(y2, 2), dt)
    out = (h if final_res == "h" else x) + (mm(s2, t["Ws2"].to(dt)) + t["bs2"].to(dt))
    return {"s1": s1, "h": h, "y2": y2, "s2": s2, "out": out}


def aud_chain(t, Mc, T, nb, dt, noise=None, **kw):
    return aud_stages(t, Mc, T, nb, dt, noise=noise, **kw)["out"]


def aud_gates(t, Mc, T, nb):
    """(fp64 reference, slack, rms gate without output rounding, calibration max, fp64 stages) of the audio tail: MARGIN x calibration
    plus one worst-placed flip of s2, the single rounded 128-value operand of the last Linear."""
    st = aud_stages(t, Mc, T, nb, torch.float64)
    c32 = aud_chain(t, Mc, T, nb, torch.float32, noise=gelu_noise((Mc, 1024)))
    cal_max, cal_rms = calibrate(c32, st["out"], 1.0)
    return st["out"], MARGIN * cal_max + flip_bound(st["s2"], t["Ws2"]), MARGIN * cal_rms, cal_max, st


def assert_store_is_rne(out_bf16, out_f32, what="bf16 store"):
    """A kernel that stores ONE fp32 value twice (fp32 and bf16) must store its round-to-nearest-even: exact equality, element by element.
    (Behind a Linear whose rounded operand can flip, the elementwise slack exceeds an ulp of the output and the rms of a truncating store
    sits on the rms gate - 4.7e-3 against 4.75e-3 at these operands; this check is what names it.)"""
    want = out_f32.detach().cpu().float().bfloat16()
    got = out_bf16.detach().cpu()
    bad = want.view(torch.int16) != got.view(torch.int16)
    if bool(bad.any()):
        r, c = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements are not the rounded fp32 output; first row {r} col {c}: "
                             f"fp32 {float(out_f32[r, c])!r} stored {float(got[r, c])!r} rounded {float(want[r, c])!r}")


def ln_raw_moment_slack(y2, A2, W):
    """What var = E[y^2] - mean^2 of fp32 sums over D values can cost behind LayerNorm -> FiLM -> SiLU -> Linear, from the fp64 y2 [M, D]:
    relative variance error D 2^-23 (1 + mean^2 / var) per row, half of it on rstd, on the pre-activation |n A2| (n the normalised
    row, A2 = gamma (1 + scale) per row), through the SiLU (SILU_LIP) and |W|."""
    y2 = y2.double()
    D = y2.shape[1]
    mean = y2.mean(-1, keepdim=True)
    var = y2.var(-1, unbiased=False, keepdim=True)
    rel_rstd = 0.5 * D * 2.0 ** -23 * (1 + mean * mean / var)
    n = (y2 - mean) / torch.sqrt(var + 1e-5)
    return (SILU_LIP * rel_rstd * (n * A2.double()).abs()) @ W.double().abs().T


# ---- audio_proj (tl_aproj_kernel) ------------------------------------------------------------------------------------------------------
def aproj_inputs(Mc, n_enc=2):
    g = torch.Generator().manual_seed(Mc + n_enc)
    return {"X": torch.randn(Mc, 256, generator=g).bfloat16(), "W": (torch.randn(n_enc, 256, 256, generator=g) / 16).bfloat16().float(),
            "b": 0.3 * torch.randn(n_enc, 256, generator=g)}


def aproj_ref(t, e, dt=torch.float64, reverse=False, bias_of=None):
    X, W = t["X"].to(dt), t["W"][e].to(dt)
    return (X.flip(1) @ W.flip(1).T if reverse else X @ W.T) + t["b"][e if bias_of is None else bias_of].to(dt)


# ---- layer-0 seed (tl_joint_kernel) ------------------------------------------------------------------------------------------------------
def joint_inputs(w, Mc, T, ldx=None, c0=0):
    """x fp32 [Mc, ldx] (the kernel multiplies bf16(x[:, c0 : c0 + w])), Wj fp32 holding bf16 values, a positional table of T + 1 rows (the
    kernel may read the first T only), the CFG-null constant."""
    ldx = ldx or w
    g = torch.Generator().manual_seed(w + Mc + T)
    return {"x": torch.randn(Mc, ldx, generator=g), "c0": c0, "w": w, "Wj": (torch.randn(512, w, generator=g) / w ** 0.5).bfloat16().float(),
            "b": 0.3 * torch.randn(512, generator=g), "pe": torch.randn(T + 1, 512, generator=g), "cnull": torch.randn(512, generator=g)}


def joint_ref(t, Mc, T, dt=torch.float64, reverse=False, pe_mod=None, kdrop=None, planes=False):
    """(conditional half, CFG-null half) = (h, h + cnull), h = bf16(x) Wj^T + bias + PE[row % T], the additions in the kernel's order.
    planes: each half rounded as hi + lo bf16 planes (the fp32 emulation).  pe_mod / kdrop: the mutants' PE modulus and first dropped column."""
    xb = rne(t["x"][:Mc, t["c0"]:t["c0"] + t["w"]], dt)
    W = t["Wj"].to(dt)
    if kdrop is not None:
        xb = xb[:, :kdrop]; W = W[:, :kdrop]
    S = xb.flip(1) @ W.flip(1).T if reverse else xb @ W.T
    h = (S + t["b"].to(dt)) + t["pe"].to(dt)[torch.arange(Mc) % (pe_mod or T)]
    hn = h + t["cnull"].to(dt)
    if planes:
        split = lambda v: v.bfloat16().to(dt) + (v - v.bfloat16().to(dt)).bfloat16().to(dt)
        h, hn = split(h), split(hn)
    return h, hn


def joint_slack(t, Mc, T):
    """Slack of the (conditional, null) halves: the fp32 accumulation over the 16 nf columns, one fp32 rounding per epilogue addition on its
    running sum (bias, PE; the null constant on the null half only), and the single hi / lo split."""
    xb = t["x"][:Mc, t["c0"]:t["c0"] + t["w"]].bfloat16().double()
    W = t["Wj"].double()
    S = xb @ W.T
    s1 = S + t["b"].double()
    h, hn = joint_ref(t, Mc, T)
    acc = accum_bound(xb, W, 16 * ((t["w"] + 15) // 16))
    add = 2.0 ** -24 * (s1.abs() + h.abs())
    return acc + add + hilo_slack(torch.zeros_like(h), h), acc + add + 2.0 ** -24 * hn.abs() + hilo_slack(torch.zeros_like(hn), hn)
