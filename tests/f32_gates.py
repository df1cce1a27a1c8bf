"""Gates, input builders and case lists for the fp32 fused launches (gemm_f32_pro.hip PRO 0 / 1 / 2 with the moments side channel,
linear_attention_f32_mfma[_sty]_kernel), derived from the arithmetic and never from a kernel's output (plain torch, CPU).  The GPU tests
(test_gpu_gemm_f32_pro.py, gp_dma_worker.py, test_gpu_f32_attention_edges.py, test_gpu_ops_golden.py "fp32-fused") and
test_f32_gates_cpu.py build their operands here, so the CPU test checks the gates on the very operands the GPU tests use.

Three evaluations per launch kind:
  ref64    the reference's op sequence in float64: F.layer_norm -> FiLM -> F.silu -> F.linear + residual; the attention as
           softmax_channels(q) (softmax_time(k)^T v) per head;
  chain32  the expression the kernel DOCUMENTS, in float32, with torch's exp and division, torch's summation order in the row moments and the
           attention, and one accumulator per output with K ascending in the Linears (_mm):
             PRO 1  the fold rstd (x W'^T - mean c) + d with two-pass row moments (W', c, d rounded to fp32 on the host, as the op takes them),
             PRO 2  normalise (two-pass moments, or the Chan combination of the group moments) -> xhat scale' + shift' -> SiLU -> Linear,
             attention + StylizationBlock front: two-pass row moments over the eight heads;
  reverse  chain32 with the K (or time) order of every accumulation flipped.
The kernel's instruction order and its hardware exp / rcp are not copied.  The one exception is onepass_moments(): the kernel's one-pass
SHIFTED moments with its accumulation grouping (8 lanes x 4 floats per K tile, 3-step butterfly), because what it tests IS a rounding
effect: shifted by the row's first element it is mutant 1 (the kernel before the fix), shifted by the mean of the first K tile it is the
documented form and must pass every gate.

Gate: EVERY element, |out - ref64| <= MARGIN x max |chain32 - ref64| (+ max |fixture - ref64| for the fixture replays, which compare with
an fp32 fixture).  The maximum runs over chain32 in BOTH summation orders: with one large term in a row (an outlier in the last real column,
300 w against a sum of a few units) the order decides whether every partial sum carries that term's ulp - the reversed chain is 4.7 x the
forward one there - and the kernel's order (K tiles ascending, two columns per MFMA step, four column groups) is neither of the two.  MARGIN = 3 for the reason given in bf16_gates.py: both differences are maxima of the same rounding distribution.  So that
the two maxima are taken over comparable populations, the calibration is never taken over fewer than CAL_ROWS rows (CAL_CLIPS clips): the
builders draw max(M, CAL_ROWS) rows of the same family, the launch gets the first M, the calibration sees all of them.

No extra slack term is added to MARGIN x calibration.  The calibration carries the fold's x W' - mean c cancellation under a large row mean
and the Chan combination of the group moments itself, because chain32 evaluates the same expressions; the hardware exp / rcp of the SiLU
(1 ulp each) is of the size of torch's own fp32 SiLU error.  Should a kernel need more at some case, the term responsible is to be named and
bounded from the fp64 operands here, as flip_bound and ln_raw_moment_slack were in bf16_gates.py - the margin stays.

Kernel / calibration ratios (max |out - ref64| over max |chain32 - ref64|, printed by every GPU test in front of its assertion) have NOT been
measured on an MI355X yet: no GPU run could be made when these tests were written.  On the CPU the emulation with the kernel's one-pass
moments (shift = first-tile mean) sits at 0.1 .. 1.5 of the calibration (median 0.8) over the CPU test's cases, the reversed-order chain at
<= 1 by construction.
"""
import functools

import torch
import torch.nn.functional as F

from bf16_gates import MARGIN, _ACTS, _check, _locate, assert_close_f32, calibrate  # noqa: F401  (re-exported for the tests)

EPS = 1e-5
CAL_ROWS = 256
CAL_CLIPS = 4
SENTINEL = 12345.0          # rows behind M of every output buffer: must come back untouched
FAMILIES = ("plain", "off+50", "off-200", "out300", "out-1e4", "out300+50", "out_last", "lowvar", "const")
OUTLIER_FAMILIES = ("out300", "out-1e4", "out300+50")


def family_rows(family, M, K, g, valid=None):
    """[M, K] rows of one input family.  valid: rows the launch sees (the constant row is placed among them)."""
    x = torch.randn(M, K, generator=g) * 1.7
    if family in ("off+50", "out300+50"):
        x += 50.0
    elif family == "off-200":
        x -= 200.0
    if family in ("out300", "out300+50"):
        x[:, 0] = 300.0
    elif family == "out-1e4":
        x[:, 0] = -1e4
    elif family == "out_last":
        x[:, K - 1] = 300.0                  # K is the real width: the last real column (of a padded segment)
    elif family == "lowvar":
        x *= 3e-3 / 1.7
    elif family == "const":
        r = const_row(valid or M)
        x[r] = x[r, 0].item()
    elif family not in FAMILIES:
        raise ValueError(family)
    return x


def const_row(valid):
    return (valid - 1) // 2


def _mm(a, w, reverse):
    """a w^T.  In fp32 with ONE accumulator per output and the K products added one at a time, K ascending (reverse: descending): the textbook
    evaluation of the sum, and the class of order a matrix-pipe K loop has.  A BLAS GEMM blocks K over its vector lanes, which shortens every
    chain of additions by the lane count: on the CPU its distance from fp64 is 2 - 3.5 x smaller than that of the single-accumulator order at
    K = 512 .. 1024, so a calibration taken from it would measure the BLAS blocking and not fp32 (fp64 evaluations use the plain product)."""
    if a.dtype != torch.float32:
        return a.flip(1) @ w.flip(1).T if reverse else a @ w.T
    acc = torch.zeros(a.shape[0], w.shape[0])
    wt = w.T.contiguous()
    for k in (range(a.shape[1] - 1, -1, -1) if reverse else range(a.shape[1])):
        acc.addcmul_(a[:, k:k + 1], wt[k][None, :])
    return acc


def _special(t):
    if t["family"] == "const":
        t["special"] = [const_row(t["M"])]
    return t


def _seed(*parts):
    """a seed that depends on the case's parameters only (hash() of a str differs from process to process)"""
    return sum((i + 1) * 7919 * (ord(c) + 1) for i, c in enumerate("|".join(str(p) for p in parts))) % (2 ** 31)


# ---- row moments ---------------------------------------------------------------------------------------------------------------------
def two_pass(x, eps=EPS, divisor=None):
    n = divisor or x.shape[1]
    mean = x.sum(-1, keepdim=True) / n
    var = ((x - mean) ** 2).sum(-1, keepdim=True) / n
    return mean, 1 / torch.sqrt(var + eps)


def onepass_moments(xp, k_real, shift, dt=torch.float32, pad_fix=True, eps=EPS):
    """gemm_f32_pro.hip's one-pass shifted moments over the zero-padded rows xp [M, K] (K a multiple of 32) with its accumulation grouping:
    lane j of 8 adds its 4 floats of every K tile ((a + b) + (c + d) for the sum, an fma chain for the squares), a 3-step butterfly joins the
    lanes, the (0 - shift) terms of the K - k_real padded columns are taken out again.  shift: "x0" (the row's first element: the kernel
    before the fix), "tile" (mean of the first K tile) or a tensor [M].  dt = float64 evaluates the same formula without the rounding."""
    M, K = xp.shape
    x = xp.to(dt).view(M, K // 32, 8, 4)
    if isinstance(shift, str):
        if shift == "x0":
            x0 = x[:, 0, 0, 0].clone()
        else:
            t = (x[:, 0, :, 0] + x[:, 0, :, 1]) + (x[:, 0, :, 2] + x[:, 0, :, 3])
            x0 = (((t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3])) + ((t[:, 4] + t[:, 5]) + (t[:, 6] + t[:, 7]))) * (1.0 / 32.0)
    else:
        x0 = shift.to(dt)
    fma = (lambda a, b, c: (a.double() * b.double() + c.double()).to(dt))
    d = x - x0[:, None, None, None]
    s1 = torch.zeros(M, 8, dtype=dt)
    s2 = torch.zeros(M, 8, dtype=dt)
    for kt in range(K // 32):
        a, b, c, e = (d[:, kt, :, i] for i in range(4))
        s1 = s1 + ((a + b) + (c + e))
        s2 = fma(a, a, fma(b, b, fma(c, c, fma(e, e, s2))))
    fly = lambda s: ((s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])) + ((s[:, 4] + s[:, 5]) + (s[:, 6] + s[:, 7]))
    a, b = fly(s1), fly(s2)
    if pad_fix:
        npad = float(K - k_real)
        a = fma(torch.full_like(x0, npad), x0, a)
        b = fma(-npad * x0, x0, b)
    invp = torch.tensor(1.0 / k_real, dtype=torch.float32).to(dt) if dt == torch.float32 else 1.0 / k_real
    dm = a * invp
    var = torch.clamp_min(fma(-dm, dm, b * invp), 0.0)
    return (x0 + dm)[:, None], (1 / torch.sqrt(var + eps))[:, None]


def group_moments(y, gs=32):
    """[M, N / gs, 2] = (mean_g, M2_g = sum (y - mean_g)^2) per group of gs columns, in y's dtype (the producer's stats_out: gs = 32)."""
    yg = y.view(y.shape[0], -1, gs)
    mg = yg.mean(-1)
    return torch.stack((mg, ((yg - mg[..., None]) ** 2).sum(-1)), -1)


def chan_combine(st, gs, K, eps=EPS, gs_factor=1.0):
    """Row moments from equal-sized group moments (Chan et al.): mean = mean of the group means, M2 = sum M2_g + gs sum (mean_g - mean)^2."""
    mu = st[..., 0].mean(-1, keepdim=True)
    m2 = st[..., 1].sum(-1, keepdim=True) + gs_factor * gs * ((st[..., 0] - mu) ** 2).sum(-1, keepdim=True)
    return mu, 1 / torch.sqrt(m2 / K + eps)


# ---- PRO 0: y = act(x W^T + b) (+ R) [+ group moments of the rows written] ---------------------------------------------------------
def pro0_inputs(M, N, K, act=0, res=True, family="plain", stats_out=False, alias=True):
    Mc = max(M, CAL_ROWS)
    g = torch.Generator().manual_seed(_seed("pro0", M, N, K, act, res, family))
    t = {"kind": "pro0", "M": M, "N": N, "K": K, "act": act, "family": family, "stats_out": stats_out, "alias": alias and res,
         "X": family_rows(family, Mc, K, g, M), "W": torch.randn(N, K, generator=g) / K ** 0.5, "b": torch.randn(N, generator=g)}
    t["R"] = torch.randn(Mc, N, generator=g) if res else None
    return _special(t)


def pro0_chain(t, dt, reverse=False, drop_tile=None):
    W = t["W"].to(dt)
    if drop_tile is not None:
        W = W.clone(); W[:, 32 * drop_tile:32 * drop_tile + 32] = 0
    y = _ACTS[t["act"]](_mm(t["X"].to(dt), W, reverse) + t["b"].to(dt))
    return y + t["R"].to(dt) if t["R"] is not None else y


# ---- PRO 1: y = act(Linear(LayerNorm(concat(x0 .. x3)))) with the LayerNorm affine folded into the weight --------------------------
def fold(W, b, gamma, beta, Kp):
    """LN(x) W^T + b = rstd (x W'^T - mean c) + d with W' = gamma (.) W (zero padded to Kp columns), c = W' 1, d = b + W beta; fp32 operands."""
    N, K = W.shape
    Wf = torch.zeros(N, Kp, dtype=torch.float64)
    Wf[:, :K] = W.double() * gamma.double()
    return Wf.float(), Wf.float().double().sum(1).float(), (b.double() + W.double() @ beta.double()).float()


def pro1_inputs(M, N, widths, k_real, act=0, family="plain", ld_extra=32):
    Mc = max(M, CAL_ROWS)
    K = sum(widths)
    g = torch.Generator().manual_seed(_seed("pro1", M, N, widths, k_real, act, family))
    X = family_rows(family, Mc, k_real, g, M)
    Xp = torch.zeros(Mc, K)
    Xp[:, :k_real] = X
    t = {"kind": "pro1", "M": M, "N": N, "K": K, "k_real": k_real, "widths": tuple(widths), "act": act, "family": family, "ld_extra": ld_extra,
         "X": X, "Xp": Xp, "W": torch.randn(N, k_real, generator=g) / k_real ** 0.5, "b": torch.randn(N, generator=g),
         "gamma": 1 + 0.3 * torch.randn(k_real, generator=g), "beta": 0.3 * torch.randn(k_real, generator=g)}
    t["Wf"], t["fc"], t["fd"] = fold(t["W"], t["b"], t["gamma"], t["beta"], K)
    return _special(t)


def pro1_segments(t, rows=None):
    """The concat segments as the launch takes them: [rows, width + ld_extra] each (strided rows; the slack columns hold NaN), None when empty."""
    segs, col = [], 0
    rows = rows or t["Xp"].shape[0]
    for w in t["widths"]:
        if w == 0:
            segs.append(None)
            continue
        s = torch.full((rows, w + t["ld_extra"]), float("nan"))
        s[:, :w] = t["Xp"][:rows, col:col + w]
        segs.append(s)
        col += w
    return segs


def pro1_ref64(t):
    k = t["k_real"]
    return _ACTS[t["act"]](F.layer_norm(t["X"].double(), (k,), t["gamma"].double(), t["beta"].double(), EPS) @ t["W"].double().T + t["b"].double())


def pro1_chain(t, dt, reverse=False, moments="two_pass", divisor=None, pad_fix=True, eps=EPS, drop_tile=None, swap=None, fc=None):
    """The fold in dtype dt.  moments: "two_pass", or onepass_moments' shift ("x0" / "tile").  The remaining arguments are the mutants'."""
    k = t["k_real"]
    xp, Wf = t["Xp"].to(dt), t["Wf"].to(dt)
    if swap is not None:                                    # two equal-width concat segments exchanged: (start a, start b, width)
        a, b, w = swap
        xp = xp.clone(); xp[:, a:a + w], xp[:, b:b + w] = t["Xp"][:, b:b + w].to(dt), t["Xp"][:, a:a + w].to(dt)
    if drop_tile is not None:
        Wf = Wf.clone(); Wf[:, 32 * drop_tile:32 * drop_tile + 32] = 0
    if moments == "two_pass":
        xr = xp[:, :k]
        mean = xr.sum(-1, keepdim=True) / (divisor or k)
        var = ((xr - mean) ** 2).sum(-1, keepdim=True) / (divisor or k)
        if divisor:                                         # (the padded zeros enter a K-divisor LayerNorm like real columns)
            var = var + (t["K"] - k) * mean ** 2 / divisor
        rstd = 1 / torch.sqrt(var + eps)
    else:
        mean, rstd = onepass_moments(xp, k, moments, dt, pad_fix=pad_fix, eps=eps)
    c = (t["fc"] if fc is None else fc).to(dt)
    return _ACTS[t["act"]](rstd * (_mm(xp, Wf, reverse) - mean * c) + t["fd"].to(dt))


# ---- PRO 2: y = Linear(SiLU(LN(x) (1 + scale) + shift)) + R, LayerNorm affine folded into the per-clip FiLM table -------------------
def pro2_inputs(M, N, K, frames, nb, family="plain", film_off=0, stat_groups=0, res=True):
    Mc = max(M, CAL_ROWS)
    g = torch.Generator().manual_seed(_seed("pro2", M, N, K, frames, nb, family, film_off, stat_groups))
    t = {"kind": "pro2", "M": M, "N": N, "K": K, "frames": frames, "nb": nb, "family": family, "film_off": film_off, "stat_groups": stat_groups, "act": 0,
         "X": family_rows(family, Mc, K, g, M), "gamma": 1 + 0.3 * torch.randn(K, generator=g), "beta": 0.3 * torch.randn(K, generator=g),
         "scale": 0.5 * torch.randn(nb, K, generator=g), "shift": 0.5 * torch.randn(nb, K, generator=g),
         "W": torch.randn(N, K, generator=g) / K ** 0.5, "b": torch.randn(N, generator=g)}
    t["R"] = torch.randn(Mc, N, generator=g) if res else None
    return pro2_finish(_special(t))


def pro2_finish(t):
    """The folded table [nb, film_off + 2 K + 8] (scale' = gamma (1 + scale), shift' = beta (1 + scale) + shift; NaN around it) and, with
    stat_groups, the group moments of the fp64 rows rounded to fp32."""
    K, off, nb = t["K"], t["film_off"], t["scale"].shape[0]
    film = torch.full((nb, off + 2 * K + 8), float("nan"))
    film[:, off:off + K] = (t["gamma"].double() * (1 + t["scale"].double())).float()
    film[:, off + K:off + 2 * K] = (t["beta"].double() * (1 + t["scale"].double()) + t["shift"].double()).float()
    t["film"] = film
    t["clip"] = (torch.arange(t["X"].shape[0]) // t["frames"]) % t["nb"]
    if t["stat_groups"]:
        t["stats"] = group_moments(t["X"].double(), K // t["stat_groups"]).float()
    return t


def pro2_ref64(t, x=None):
    K = t["K"]
    x = t["X"].double() if x is None else x
    hn = F.layer_norm(x, (K,), t["gamma"].double(), t["beta"].double(), EPS)
    y = F.silu(hn * (1 + t["scale"].double()[t["clip"]]) + t["shift"].double()[t["clip"]]) @ t["W"].double().T + t["b"].double()
    return y + t["R"].double() if t["R"] is not None else y


def pro2_chain(t, dt, reverse=False, x=None, moments="two_pass", eps=EPS, film_rows=None, drop_tile=None, gs_factor=1.0, stats=None):
    """x: the rows (default t["X"]; the side-channel chain passes its producer's output).  With t["stat_groups"] the row moments are the Chan
    combination of the group moments of x taken in dt (or of `stats`)."""
    K, off = t["K"], t["film_off"]
    x = (t["X"] if x is None else x).to(dt)
    W = t["W"].to(dt)
    if drop_tile is not None:
        W = W.clone(); W[:, 32 * drop_tile:32 * drop_tile + 32] = 0
    if t["stat_groups"]:
        gs = K // t["stat_groups"]
        mean, rstd = chan_combine(group_moments(x, gs) if stats is None else stats.to(dt), gs, K, eps, gs_factor)
    elif moments == "two_pass":
        mean, rstd = two_pass(x, eps)
    else:
        mean, rstd = onepass_moments(x, K, moments, dt, eps=eps)
    f = t["film"].to(dt)[t["clip"] if film_rows is None else film_rows]
    s = F.silu((x - mean) * rstd * f[:, off:off + K] + f[:, off + K:off + 2 * K])
    y = _mm(s, W, reverse) + t["b"].to(dt)
    return y + t["R"].to(dt) if t["R"] is not None else y


def neighbour_rows(t):
    """mutant: the last frame of every clip takes the next clip's FiLM row"""
    rows = torch.arange(t["X"].shape[0])
    return torch.where(rows % t["frames"] == t["frames"] - 1, (t["clip"] + 1) % t["nb"], t["clip"])


# ---- the moments side channel: PRO 0 producer (stats_out) -> PRO 2 consumer (stats) -------------------------------------------------
def side_inputs(M, K1, D, frames, nb, offset=0.0):
    Mc = max(M, CAL_ROWS)
    g = torch.Generator().manual_seed(_seed("side", M, K1, D, frames, nb, offset))
    prod = {"kind": "pro0", "M": M, "N": D, "K": K1, "act": 0, "family": "plain", "stats_out": True, "alias": False, "R": None,
            "X": torch.randn(Mc, K1, generator=g), "W": torch.randn(D, K1, generator=g) / K1 ** 0.5, "b": torch.randn(D, generator=g) + offset}
    t = {"kind": "side", "M": M, "N": D, "K": D, "frames": frames, "nb": nb, "family": "plain", "film_off": 0, "stat_groups": D // 32, "act": 0,
         "prod": prod, "X": torch.zeros(Mc, D), "gamma": 1 + 0.3 * torch.randn(D, generator=g), "beta": 0.3 * torch.randn(D, generator=g),
         "scale": 0.5 * torch.randn(nb, D, generator=g), "shift": 0.5 * torch.randn(nb, D, generator=g),
         "W": torch.randn(D, D, generator=g) / D ** 0.5, "b": torch.randn(D, generator=g), "R": torch.randn(Mc, D, generator=g)}
    t = pro2_finish(dict(t, stat_groups=0))
    t["stat_groups"] = D // 32
    return t


def side_chain(t, dt, reverse=False, **kw):
    """ref64 (dt = float64): LayerNorm of the fp64 producer rows; chain32: producer in fp32, its group moments, Chan combination."""
    y2 = pro0_chain(t["prod"], dt, reverse)
    if dt == torch.float64 and not kw:
        return pro2_ref64(t, y2)
    return pro2_chain(t, dt, reverse, x=y2, **kw)


# ---- fp32 linear attention (D = 512, eight 64-channel heads) [+ StylizationBlock front] ---------------------------------------------
ATTN_FAMILIES = ("plain", "v_out", "v_small", "k_sat")


def attn_inputs(nb, T, family="plain", sty=False):
    """qkv [max(nb, CAL_CLIPS), T + 1, 1536]: the launch gets the first nb clips and the first T frames of each (frame T exists for the
    T + 1 mutant only); sty: three-and-more distinct folded FiLM rows [clips, 1024]."""
    nbc = max(nb, CAL_CLIPS)
    g = torch.Generator().manual_seed(_seed("attn", nb, T, family, sty))
    qkv = torch.randn(nbc, T + 1, 1536, generator=g) * 1.5
    if family == "v_out":
        qkv[:, :, 1024 + 7] = 300.0
    elif family == "v_small":
        qkv[:, :, 1024:] *= 1e-3
    elif family == "k_sat":
        qkv[:, T // 2, 512:1024] += 40.0
    elif family != "plain":
        raise ValueError(family)
    t = {"kind": "attn_sty" if sty else "attn", "nb": nb, "T": T, "family": family, "qkv": qkv}
    if sty:
        gamma, beta = 1 + 0.3 * torch.randn(512, generator=g), 0.3 * torch.randn(512, generator=g)
        scale, shift = 0.5 * torch.randn(nbc, 512, generator=g), 0.5 * torch.randn(nbc, 512, generator=g)
        t["film"] = torch.cat(((gamma.double() * (1 + scale.double())).float(), (beta.double() * (1 + scale.double()) + shift.double()).float()), 1)
    return t


def attn_chain(t, dt, reverse=False, extra_frame=False, moment_heads=8, film_rows=None):
    """[clips, T, 512].  reverse: the time order of the k-softmax and of A = k^T v flipped.  extra_frame (mutant): the time-softmax and A take
    T + 1 frames.  moment_heads (mutant): the row moments of the front over that many heads (64 channels each) instead of all eight."""
    T, hd, H = t["T"], 64, 8
    qkv = t["qkv"].to(dt)
    n = T + 1 if extra_frame else T
    q, k, v = (qkv[:, :, i * 512:(i + 1) * 512].reshape(qkv.shape[0], T + 1, H, hd) for i in range(3))
    k, v = k[:, :n], v[:, :n]
    if reverse:
        k, v = k.flip(1), v.flip(1)
    A = torch.einsum("bnhd,bnhl->bhdl", k.softmax(dim=1), v)
    y = torch.einsum("bnhd,bhdl->bnhl", q[:, :T].softmax(dim=-1), A).reshape(qkv.shape[0], T, 512)
    if t["kind"] == "attn":
        return y
    w = 64 * moment_heads
    yg = y.view(y.shape[0], T, 512 // w, w)
    mean = yg.sum(-1, keepdim=True) / w
    xhat = ((yg - mean) / torch.sqrt(((yg - mean) ** 2).sum(-1, keepdim=True) / w + EPS)).reshape(y.shape)
    f = t["film"].to(dt)[torch.arange(qkv.shape[0]) % t["nb"] if film_rows is None else film_rows][:, None, :]
    return F.silu(xhat * f[..., :512] + f[..., 512:])


def attention_core(qkv, reverse=False):
    """[nb, T, 1536] -> [nb, T, 512]: softmax_channels(q) (softmax_time(k)^T v) per 64-channel head, in qkv's dtype"""
    nb, T, _ = qkv.shape
    q, k, v = (qkv[:, :, i * 512:(i + 1) * 512].reshape(nb, T, 8, 64) for i in range(3))
    if reverse:
        k, v = k.flip(1), v.flip(1)
    A = torch.einsum("bnhd,bnhl->bhdl", k.softmax(dim=1), v)
    return torch.einsum("bnhd,bhdl->bnhl", q.softmax(dim=-1), A).reshape(nb, T, 512)


# ---- one interface over the launch kinds -----------------------------------------------------------------------------------------------
def ref64(t):
    k = t["kind"]
    if k == "pro0":
        return pro0_chain(t, torch.float64)
    if k == "pro1":
        return pro1_ref64(t)
    if k == "pro2":
        return pro2_ref64(t)
    if k == "side":
        return side_chain(t, torch.float64)
    return attn_chain(t, torch.float64).reshape(-1, 512)


def chain(t, dt=torch.float32, **kw):
    k = t["kind"]
    fn = {"pro0": pro0_chain, "pro1": pro1_chain, "pro2": pro2_chain, "side": side_chain}.get(k)
    return fn(t, dt, **kw) if fn else attn_chain(t, dt, **kw).reshape(-1, 512)


def valid_rows(t):
    """rows of ref64 / chain the launch computes"""
    if t["kind"] in ("attn", "attn_sty"):
        return torch.arange(t["nb"] * t["T"])
    return torch.arange(t["M"])


def gate(t):
    """(ref64 over all calibration rows, allowance [rows, 1] = MARGIN x max |chain32 - ref64| over both summation orders, calibration maximum).
    The all-constant row of the "const" family is a population of its own (rstd = eps^-1/2 = 316 multiplies the round-off of x W' - mean c,
    two to three orders above every other row): it gets the allowance of its own N elements, and the other rows are not loosened by it."""
    if "_gate" not in t:
        ref = ref64(t)
        cols = t.get("cal_cols")
        if cols is None:
            err = torch.maximum(*((chain(t, reverse=r).double() - ref).abs() for r in (False, True)))
        else:
            # a PRO 0 launch with thousands of output columns (the FiLM table's N = 16 384): the single-accumulator fp32 chain costs K passes
            # over [rows, N], so the calibration is taken over a SAMPLE of the columns (every column draws W and b from one distribution).  A
            # maximum over fewer elements is never larger than the maximum over all of them: the allowance can only shrink by this.
            assert t["kind"] == "pro0" and len(cols) >= 512, "column-sampled calibration: PRO 0, at least 512 columns"
            s = {k: v for k, v in t.items() if not k.startswith("_") and k != "cal_cols"}
            s.update(W=t["W"][cols], b=t["b"][cols], N=len(cols), R=None if t["R"] is None else t["R"][:, cols])
            err = torch.maximum(*((chain(s, reverse=r).double() - ref[:, cols]).abs() for r in (False, True)))
        rest = torch.ones(err.shape[0], dtype=torch.bool)
        rest[t.get("special", [])] = False
        cal = float(err[rest].max())
        allow = torch.full((err.shape[0], 1), MARGIN * cal, dtype=torch.float64)
        for r in t.get("special", []):
            allow[r] = MARGIN * float(err[r].max())
        t["_gate"] = (ref, allow, cal)
    return t["_gate"]


def stats_gate(t):
    """Group moments a PRO 0 launch leaves (stats_out): reference = fp64 moments of the fp64 rows; allowance = MARGIN x the difference of the
    fp32 moments of the fp32 chain from it, per component (mean_g, M2_g)."""
    if "_sgate" not in t:
        ref = group_moments(pro0_chain(t, torch.float64))
        d = (group_moments(pro0_chain(t, torch.float32)).double() - ref).abs()
        t["_sgate"] = (ref, MARGIN * d[..., 0].max().item(), MARGIN * d[..., 1].max().item())
    return t["_sgate"]


def check(t, out, what=None, extra=0.0):
    """Gate the launch's output rows (a [rows >= valid, N] tensor; only the valid rows are compared).  Returns kernel / calibration."""
    ref, allow, cal = gate(t)
    rows = valid_rows(t)
    o = out.detach().cpu().reshape(-1, ref.shape[-1])[:len(rows)]
    frames = t.get("frames", t.get("T", 0))
    assert_close_f32(o, ref[rows], (allow[rows] + extra).expand(len(rows), ref.shape[-1]), what or t.get("name", t["kind"]), frames=frames, nb=t.get("nb", 0))
    return float(((o.double() - ref[rows]).abs() / allow[rows].clamp_min(1e-300)).max()) * MARGIN


def ratio(t, out):
    """kernel / calibration without asserting (printed in front of every assertion): the largest |out - ref64| over its row's calibration"""
    ref, allow, cal = gate(t)
    rows = valid_rows(t)
    o = out.detach().cpu().reshape(-1, ref.shape[-1])[:len(rows)].double()
    return float(((o - ref[rows]).abs() / allow[rows].clamp_min(1e-300)).max()) * MARGIN, cal


# ---- case lists (shared by the CPU test, the in-process GPU tests and gp_dma_worker.py) -----------------------------------------------
GRID_M = (1, 63, 64, 65, 448, 449, 64 * 11 + 5)
GRID_N = (4, 60, 64, 68, 100, 1536)
GRID_K = (32, 64, 96, 512, 1024)
FAMILY_WIDTHS = (512, 256, 128, 64)          # feat_proj.1 of the BEAT gesture encoder: 947 real columns, 13 zero-padded ones
PRO2_CLIPS = ((1, 5), (11, 7), (34, 3), (88, 2))


def _cases():
    c = {}
    # the small-shape grid: one case per (PRO, M, N, K); PRO 0 alternates activation / residual with the shape, PRO 2 its clip layout
    for im, M in enumerate(GRID_M):
        for i_n, N in enumerate(GRID_N):
            for ik, K in enumerate(GRID_K):
                j = im + i_n + ik
                c[f"p0-grid-{M}x{N}x{K}"] = (pro0_inputs, (M, N, K), {"act": j % 3, "res": j % 2 == 0})
                c[f"p1-grid-{M}x{N}x{K}"] = (pro1_inputs, (M, N, (K, 0, 0, 0), K), {"act": j % 2, "ld_extra": 32 * (j % 2)})
                c[f"p2-grid-{M}x{N}x{K}"] = (pro2_inputs, (M, N, K) + PRO2_CLIPS[j % 4], {})
    # PRO 0: residual aliasing / not aliasing the output, no residual, SiLU and GELU, group moments of the written rows
    for act in (0, 1, 2):
        for res, alias in ((False, False), (True, True), (True, False)):
            c[f"p0-act{act}-res{int(res)}-alias{int(alias)}"] = (pro0_inputs, (130, 192, 96), {"act": act, "res": res, "alias": alias})
    for N in (64, 128, 512):
        c[f"p0-stats-{N}"] = (pro0_inputs, (130, N, 96), {"stats_out": True, "res": False})
        c[f"p0-stats-{N}-res"] = (pro0_inputs, (449, N, 1024), {"stats_out": True, "res": True})
    # PRO 1: concat segments
    for widths, k_real in (((32, 32, 32, 32), 97), ((32, 32, 32, 32), 127), ((32, 32, 32, 32), 128), ((512, 0, 128, 64), 690), ((512, 0, 128, 64), 704),
                           ((512, 256, 0, 0), 768), ((512, 256, 128, 128), 999)):
        for act in (0, 1):
            c[f"p1-seg-{'_'.join(map(str, widths))}-{k_real}-act{act}"] = (pro1_inputs, (130, 192, widths, k_real), {"act": act})
    # every input family: PRO 1 over the padded concat and over one 512-wide segment (q|k|v), PRO 2 with its own moments
    for fam in FAMILIES:
        c[f"p1-fam-{fam}-947"] = (pro1_inputs, (200, 192, FAMILY_WIDTHS, 947), {"act": 1, "family": fam})
        c[f"p1-fam-{fam}-512"] = (pro1_inputs, (200, 128, (512, 0, 0, 0), 512), {"act": 0, "family": fam})
        c[f"p2-fam-{fam}-512"] = (pro2_inputs, (200, 128, 512, 34, 3), {"family": fam})
        c[f"p2-fam-{fam}-1024"] = (pro2_inputs, (130, 64, 1024, 11, 7), {"family": fam, "film_off": 4 * 1024})
    # PRO 2: clip layouts (a 64-row block spans 1 .. 64 clips), table at a column offset, group moments built from the fp64 rows
    for frames, nb in PRO2_CLIPS:
        c[f"p2-clips-{frames}x{nb}"] = (pro2_inputs, (449, 128, 128, frames, nb), {"film_off": 8})
    for G, K in ((1, 96), (2, 64), (4, 128), (16, 512), (1, 512), (4, 1024)):
        c[f"p2-stats-{G}x{K // G}"] = (pro2_inputs, (130, 128, K, 11, 7), {"stat_groups": G})
        c[f"p2-stats-{G}x{K // G}-off"] = (pro2_inputs, (130, 128, K, 34, 3), {"stat_groups": G, "family": "off+50"})
    # the side channel end to end: producer N = 64 / 128 / 512 -> 2 / 4 / 16 groups
    for D in (64, 128, 512):
        c[f"side-{D}"] = (side_inputs, (130, 96, D, 11, 7), {})
    c["side-512-off"] = (side_inputs, (311, 1024, 512, 34, 9), {"offset": 30.0})
    return c


CASES = _cases()
ATTN_T = (1, 2, 31, 32, 33, 35, 36, 37, 63, 64, 65, 95, 96, 97)
ATTN_STY_T = (1, 2, 31, 32, 33, 36, 37, 63, 64)


@functools.lru_cache(maxsize=4)          # (tests that share a case run next to each other; the big grid cases are not kept)
def case(name):
    fn, a, kw = CASES[name]
    t = fn(*a, **kw)
    t["name"] = name
    if t["kind"] == "side":
        t["prod"]["name"] = name + "/producer"
    return t


def case_names(prefix=""):
    return [n for n in CASES if n.startswith(prefix)]
