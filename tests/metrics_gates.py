"""Builders, references and gates for the op-level tests of the validation metrics (csrc/pose_encoder.hip conv_gemm_f32_kernel through
dsh_op_conv_gemm_f32, csrc/metrics.hip through dsh_op_batch_metrics, the FGD encoder through metrics.HalfEmbeddingNet), in the form of
f32_gates.py: derived from the arithmetic and never from a kernel's output (plain torch / numpy, CPU).  test_gpu_conv_gemm.py,
test_gpu_metrics_edges.py and test_gpu_fgd_encoder_edges.py build their operands here, test_metrics_gates_cpu.py shows on the same
operands that the gates accept faithful emulations and reject subtly wrong kernels.

Conv (one launch = one Conv1d stage as an implicit GEMM over channels-last clips):
  ref64    ONE float64 matmul of the unfolded slices x[b, s t : s t + k, :] against W[:, :Kreal], plus bias and LeakyReLU(0.2);
  chain32  the same in float32 through f32_gates._mm (one accumulator per output), in both K orders;
  gate     every element |out - ref64| <= MARGIN x max |chain32 - ref64|, the maximum over both orders and over never fewer than CAL_ROWS
           rows of the same family (the builder draws more clips than the launch gets where B x Tout is smaller).
  The `ints` family (small integers in X, W and the bias: every partial sum is exact in fp32 in any order) has no gate: the output must
  equal ref64 BIT FOR BIT.  Its LeakyReLU slope is float32(0.2), the constant the fp32 epilogue multiplies by; an exact integer times that
  constant, rounded once, is what both sides compute.

PCK: pck_emul is the reference's float32 arithmetic spelled out in numpy (individually rounded products, (p0 + p1) + p2, the correctly
rounded root float32(sqrt(float64(s))) < 0.5).  The `threshold` family puts every joint ON the threshold: n unit directions times 0.5 rounded
to float32 as `outputs`, `motions` = 0; its second form offsets both tensors by 37.25 (the float32 subtraction then decides what the
squares see).  On 2 M such triplets (test_metrics_gates_cpu.py measures it again on a sample): 17 % have s equal to the float32 just below
0.25, 76 % s = 0.25 exactly, 5 % the float32 just above; 11 % change side when either addition is contracted into an FMA and 32 %
disagree with the float64 root.  For joint_dim 1 the family is 0.5, -0.5 and the float32 neighbours of both, tiled.

MSE gate (derived): sq_sum against the exactly rounded (math.fsum) float64 sum of the squares of the float32 differences, relative
n_elems x 2^-53: the squares are exact in fp64, all terms are non-negative, and a sum of n such terms in fp64 in ANY order is within
(n - 1) 2^-53 of the exact one.
Diversity gate (derived): per group, relative b_div x 2^-24: each |v_i - v_j| is rounded once (2^-24), at most b_div - 1 non-negative terms are
added in fp32 (b_div - 2 roundings of 2^-24), everything behind is fp64.  div_kernel_order() evaluates exactly that order on the CPU and
test_metrics_gates_cpu.py checks that it stays inside the gate at every family and shape the GPU test uses.

Measured on an MI355X (every GPU test prints its figure in front of the assertion): conv kernel / calibration 0.03 - 1.11 over
the 64 gated launches (the gate allows MARGIN = 3), the 20 integer launches exact, the two kernel instantiations bit-identical on shared
rows; sq_sum at most 0.001 of its gate, every PCK count exact (789 of the 4 096 threshold joints; an FMA in either addition gives 762 /
992, a root one ulp high 78), diversity at most 0.43 of its gate; encoder latents 0.33 - 0.85 of the calibration.  In the offset form of
the threshold family the differences are multiples of 2^-18 and few joints stay within an ulp of 0.25: it tests the subtraction, and only
the unshifted form is sensitive to every mutant.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from f32_gates import CAL_ROWS, MARGIN, SENTINEL, _mm, _seed, assert_close_f32  # noqa: F401  (re-exported for the tests)

NAN = float("nan")
SLOPE = 0.2
SLOPE32 = float(np.float32(0.2))
X_TAIL = 64                     # NaN floats behind the last clip of X (more than any K pad: Kp - Kreal < 32)
Y_TAIL_ROWS = 8                 # SENTINEL rows behind the last clip of Y
CONV_FAMILIES = ("plain", "off+50", "out_last", "ints")


# ---- conv: one launch ---------------------------------------------------------------------------------------------------------------------
def conv_inputs(B, Tin, Cin, ks, stride, N, family="plain", leaky=1, x_gap=0, y_gap=0, ldw_extra=0):
    """One Conv1d launch over B channels-last clips [Tin, Cin].  x_gap / y_gap: floats between the clips of X / behind the Tout x N outputs
    of a clip in Y.  The tensors hold max(B, clips for CAL_ROWS rows) clips of the family: the launch gets the first B."""
    Tout = (Tin - ks) // stride + 1
    assert Tout >= 1 and x_gap % 4 == 0 and y_gap % 4 == 0
    Kreal = ks * Cin
    Bc = max(B, -(-CAL_ROWS // Tout))
    g = torch.Generator().manual_seed(_seed("conv", B, Tin, Cin, ks, stride, N, family, leaky, x_gap, y_gap))
    if family == "ints":
        X = torch.randint(-8, 9, (Bc, Tin, Cin), generator=g).float()
        W = torch.randint(-4, 5, (N, Kreal), generator=g).float()
        b = torch.randint(-50, 51, (N,), generator=g).float()
    else:
        X = torch.randn(Bc, Tin, Cin, generator=g)
        W = torch.randn(N, Kreal, generator=g) / Kreal ** 0.5
        b = torch.randn(N, generator=g)
        if family == "off+50":
            X += 50.0
        elif family == "out_last":
            X[:, ks - 1::stride, Cin - 1][:, :Tout] = 300.0       # the last real k of EVERY row: right at the mask boundary
        elif family != "plain":
            raise ValueError(family)
    return {"kind": "conv", "B": B, "Bc": Bc, "Tin": Tin, "Cin": Cin, "ks": ks, "stride": stride, "N": N, "family": family, "leaky": int(leaky),
            "Tout": Tout, "M": B * Tout, "Kreal": Kreal, "Kp": -(-Kreal // 32) * 32, "x_step": stride * Cin, "x_clip": Tin * Cin + x_gap,
            "y_clip": Tout * N + y_gap, "ldw": -(-Kreal // 32) * 32 + ldw_extra, "X": X, "W": W, "b": b}


def conv_rows(t, dt):
    """[Bc * Tout, Kreal]: the im2col rows, row (b, t) = the contiguous slice x[b, s t : s t + k, :]"""
    X = t["X"].to(dt)
    return X.unfold(1, t["ks"], t["stride"]).permute(0, 1, 3, 2).reshape(-1, t["Kreal"])


def _act(y, t, slope):
    return F.leaky_relu(y, slope) if t["leaky"] else y


def conv_chain(t, dt, reverse=False):
    slope = SLOPE32 if t["family"] == "ints" else SLOPE
    return _act(_mm(conv_rows(t, dt), t["W"].to(dt), reverse) + t["b"].to(dt), t, slope)


def conv_ref64(t):
    return conv_chain(t, torch.float64)


def conv_x_flat(t, clips=None, dt=torch.float32):
    """The X buffer of the launch: [clips * x_clip + X_TAIL] floats, NaN everywhere but where some output's Kreal window reads - the gap
    between the clips, frames no window covers (stride 2) and the tail behind the last clip are NaN."""
    B = clips or t["B"]
    flat = torch.full((B * t["x_clip"] + X_TAIL,), NAN, dtype=dt)
    idx = conv_index(t, B, t["x_clip"], t["x_step"], t["Kreal"]).reshape(-1)
    flat[idx] = conv_rows(t, dt)[:B * t["Tout"]].reshape(-1)
    return flat


def conv_index(t, B, x_clip, x_step, kread):
    """[B * Tout, kread] float offsets into the X buffer: b x_clip + t x_step + k (the kernel's A row base plus k)"""
    b = torch.arange(B)[:, None, None] * x_clip
    r = torch.arange(t["Tout"])[None, :, None] * x_step
    return (b + r + torch.arange(kread)[None, None, :]).reshape(B * t["Tout"], kread)


def conv_w_padded(t, dt=torch.float32):
    """[N, ldw]: K zero padded to Kp, NaN in the ldw - Kp columns behind (never read)"""
    W = torch.full((t["N"], t["ldw"]), NAN, dtype=dt)
    W[:, :t["Kp"]] = 0
    W[:, :t["Kreal"]] = t["W"].to(dt)
    return W


def conv_mutant(t, mutant):
    """[M, N] float64: the launch with ONE thing wrong, evaluated by addressing the launch's own X buffer as the kernel does.
      drop_piece   the last 16-byte piece of Kreal is not loaded (k >= Kreal - 4 staged as zero)
      read_pad     the K pad of the activation side is read instead of masked (0 x NaN behind the row)
      step_cin     x_step = Cin on a stride-2 conv
      slope_001    LeakyReLU slope 0.01
      bias_quad    the bias quad taken four columns further (wrapping at N)
      clip_base    the clip base b * Tin * Cin: the gap in x_clip ignored"""
    f64 = torch.float64
    B, Kreal, Kp = t["B"], t["Kreal"], t["Kp"]
    flat = conv_x_flat(t, dt=f64)
    W = conv_w_padded(t, f64)[:, :Kp]
    x_clip, x_step, kread = t["x_clip"], t["x_step"], Kreal
    if mutant == "read_pad":
        kread = Kp
    elif mutant == "step_cin":
        x_step = t["Cin"]
    elif mutant == "clip_base":
        x_clip = t["Tin"] * t["Cin"]
    rows = flat[conv_index(t, B, x_clip, x_step, kread)]
    if mutant == "drop_piece":
        rows = rows.clone()
        rows[:, Kreal - 4:] = 0
    b = t["b"].to(f64)
    if mutant == "bias_quad":
        b = b.roll(-4)
    slope = 0.01 if mutant == "slope_001" else SLOPE
    return _act(rows @ W[:, :kread].T + b, t, slope)


CONV_MUTANTS = {
    "drop_piece": lambda t: True,
    "read_pad": lambda t: t["Kp"] > t["Kreal"],
    "step_cin": lambda t: t["stride"] == 2 and t["Tout"] > 1,
    "slope_001": lambda t: t["leaky"] == 1,
    "bias_quad": lambda t: t["N"] > 4,
    "clip_base": lambda t: t["x_clip"] > t["Tin"] * t["Cin"] and t["B"] > 1,
}


def conv_gate(t):
    """(ref64 [Bc Tout, N], calibration = max |chain32 - ref64| over both K orders and all Bc x Tout rows)"""
    if "_gate" not in t:
        ref = conv_ref64(t)
        if t["family"] == "ints":
            # every sum is an integer below 2^24 (exact in fp32 in any order); times float32(0.2) it has 48 bits in fp64 and is rounded ONCE
            absmax = float((conv_rows(t, torch.float64).abs() @ t["W"].double().abs().T).max() + t["b"].abs().max())
            assert absmax < 2 ** 24
            t["_gate"] = (ref.float().double(), 0.0)
        else:
            assert t["Bc"] * t["Tout"] >= CAL_ROWS
            cal = max(float((conv_chain(t, torch.float32, reverse=r).double() - ref).abs().max()) for r in (False, True))
            t["_gate"] = (ref, cal)
    return t["_gate"]


def conv_ratio(t, out):
    """'exact' / 'NOT exact' for the ints family, else kernel / calibration as a string (printed in front of every assertion)"""
    ref, cal = conv_gate(t)
    o = out.detach().cpu().reshape(t["M"], t["N"])
    if t["family"] == "ints":
        return "exact" if torch.equal(o, ref[:t["M"]].float()) else "NOT exact"
    return f"{float((o.double() - ref[:t['M']]).abs().max()) / cal:.3f} (calibration {cal:.2e})"


def conv_check(t, out, what=None):
    """Gate the [M, N] output of the launch on every element (bit for bit in the ints family)."""
    ref, cal = conv_gate(t)
    o = out.detach().cpu().reshape(t["M"], t["N"])
    what = what or t.get("name", "conv")
    assert_close_f32(o, ref[:t["M"]], 0.0 if t["family"] == "ints" else MARGIN * cal, what, frames=t["Tout"], nb=t["B"])
    if t["family"] == "ints":
        assert torch.equal(o, ref[:t["M"]].float()), what


# M of the dispatch rules at N = 68 (nt_n = 2), K = 24 (Cin 8, kernel 3, stride 1): name -> (B, Tin)
CONV_DISPATCH = {448: (1, 450),      # <1,1>, nt_m 7: plain block order
                 449: (1, 451),      # nt_m 8: XCD order
                 513: (3, 173),      # nt_m 9: seven padded blocks per N tile return early
                 2047: (23, 91),     # the last M of <1,1>
                 2048: (2, 1026),    # <2,1>, nt_m 16
                 2049: (3, 685)}     # nt_m 17, padded
CONV_N = (4, 60, 64, 68, 300)
# Kreal -> (Cin, ks, stride): 4 one piece per row; 28 / 32 / 36 around one K tile (36: a second tile holding one piece); 696 -> Kp 704
# (layer 0 of SHOW), 1200 -> Kp 1216
CONV_K = {4: (4, 1, 1), 28: (4, 7, 1), 32: (8, 4, 2), 36: (12, 3, 1), 696: (232, 3, 1), 1200: (400, 3, 1)}
CONV_GEOM = ((3, 1, None), (4, 2, None), (3, 1, 1))          # (ks, stride, Tout or None)


def _conv_cases():
    c = {}
    for i, (M, (B, Tin)) in enumerate(CONV_DISPATCH.items()):
        c[f"dispatch-M{M}"] = ((B, Tin, 8, 3, 1, 68), {"family": CONV_FAMILIES[i % 4], "leaky": (i // 3) % 2, "y_gap": 4 * (i % 2)})
    # every width against every K; family, batch, rows (one row, part of a tile, more than one block), gaps and activation cycle
    for i, N in enumerate(CONV_N):
        for j, (K, (Cin, ks, s)) in enumerate(CONV_K.items()):
            n = i + j
            Tout = (1, 23, 70)[n % 3]
            c[f"width-N{N}-K{K}"] = ((1 + 2 * (n % 2), (Tout - 1) * s + ks, Cin, ks, s, N),
                                     {"family": CONV_FAMILIES[n % 4], "leaky": (n // 4 + n) % 2, "x_gap": 8 * ((n // 3) % 2), "y_gap": 12 * (n % 2),
                                      "ldw_extra": 4 * ((n // 4) % 2)})
    n = 0
    for ks, s, tout in CONV_GEOM:
        for B in (1, 3):
            for x_gap in (0, 8):
                for y_gap in (0, 12):
                    for leaky in (0, 1):
                        Tin = ks if tout == 1 else 40 + (n % 2)            # (Tin 41 with stride 2: the last frame is covered by no window)
                        c[f"geom-k{ks}s{s}{'-one' if tout else ''}-B{B}-xg{x_gap}-yg{y_gap}-act{leaky}"] = (
                            (B, Tin, 8, ks, s, 68), {"family": CONV_FAMILIES[(n // 2 + n // 8) % 4], "leaky": leaky, "x_gap": x_gap, "y_gap": y_gap})
                        n += 1
    return c


CONV_CASES = _conv_cases()


@functools.lru_cache(maxsize=None)      # (90 small cases: the CPU test visits each once per mutant)
def conv_case(name):
    a, kw = CONV_CASES[name]
    t = conv_inputs(*a, **kw)
    t["name"] = name
    return t


# ---- PCK ----------------------------------------------------------------------------------------------------------------------------------
F32 = np.float32
BELOW_QUARTER = np.nextafter(F32(0.25), F32(0))
ABOVE_QUARTER = np.nextafter(F32(0.25), F32(1))


def _fma32(a, b, c):
    """float32(a b + c) with one rounding (the exact product of two float32 fits a float64; the float64 sum is within 2^-53 of exact)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def pck_sums(outputs, motions, joint_dim, contract=0):
    """s [n_joints] float32 as the reference forms it: d = o - m, individually rounded products, (p0 + p1) + p2.
    contract (mutants): 1 = the first addition fused with the product d1 d1, 2 = the second with d2 d2."""
    d = (np.asarray(outputs, dtype=F32) - np.asarray(motions, dtype=F32)).reshape(-1, joint_dim)
    p = d * d
    if joint_dim == 1:
        return p[:, 0]
    s01 = _fma32(d[:, 1], d[:, 1], p[:, 0]) if contract == 1 else p[:, 0] + p[:, 1]
    return _fma32(d[:, 2], d[:, 2], s01) if contract == 2 else s01 + p[:, 2]


def pck_hits(s, le=False, sqrt_high=False):
    """float32(sqrt(float64(s))) < 0.5.  Mutants: <= in place of <; a root one ulp high at s = the float32 below 0.25 (its correctly rounded
    root is the float32 below 0.5, one ulp up is 0.5)."""
    root = np.sqrt(s.astype(np.float64)).astype(F32)
    if sqrt_high:
        root = np.where(s == BELOW_QUARTER, np.nextafter(root, F32(1)), root)
    return root <= F32(0.5) if le else root < F32(0.5)


def pck_emul(outputs, motions, joint_dim, contract=0, le=False, sqrt_high=False):
    return int(pck_hits(pck_sums(outputs, motions, joint_dim, contract), le, sqrt_high).sum())


def pck_restated(outputs, motions, joint_dim):
    """The reference's lines, restated directly in numpy float32: sqrt(sum(diff^2, last axis)) < 0.5 over [..., joints, joint_dim]"""
    diff = np.asarray(outputs, dtype=F32) - np.asarray(motions, dtype=F32)
    diff = diff.reshape(-1, joint_dim)
    return int((np.sqrt(np.sum(diff ** 2, axis=1)) < 0.5).sum())


def threshold_joints(n, seed=0, offset=0.0):
    """(outputs, motions) [n, 3] float32: n unit directions times 0.5 rounded to float32 against 0; offset: both tensors moved by it in
    float32 (the subtraction then returns the offset sum's rounding of the direction)."""
    g = np.random.default_rng(_seed("threshold", n, seed))
    v = g.standard_normal((n, 3))
    v = (0.5 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    return (v + F32(offset)).astype(F32), np.full((n, 3), offset, dtype=F32)


def threshold_scalars(n):
    """joint_dim 1: 0.5, -0.5 and the float32 neighbours of both, tiled to n elements"""
    h = F32(0.5)
    vals = np.array([h, -h, np.nextafter(h, F32(0)), np.nextafter(h, F32(1)), -np.nextafter(h, F32(0)), -np.nextafter(h, F32(1))], dtype=F32)
    return np.resize(vals, n), np.zeros(n, dtype=F32)


# ---- MSE / diversity ----------------------------------------------------------------------------------------------------------------------
# (B, T, C, joint_dim, b_div) of test_gpu_metrics_edges.py
METRIC_SHAPES = ((2, 1, 3, 3, 2),
                 (3, 1, 4, 1, 2),          # the remainder clip is dropped
                 (5, 7, 36, 3, 2),         # two groups, a remainder, 252 columns: less than one chunk
                 (4, 1, 256, 1, 4),        # exactly one chunk
                 (4, 1, 257, 1, 2),        # one column in a second chunk
                 (64, 3, 192, 3, 64),      # 64 KB of dynamic LDS
                 (65, 3, 192, 3, 65),      # just above
                 (130, 2, 6, 3, 128),      # the limit, remainder 2
                 (13, 88, 232, 1, 13))     # more joints than 1024 x 256 threads: the grid-stride loop
METRIC_FAMILIES = ("plain", "scales")


def metric_inputs(B, T, C, joint_dim, b_div, family="plain"):
    """(outputs, motions) [B, T, C] float32.  scales: a column of 1e4 next to a column of 1e-3 (sums over pairs of very different size)."""
    g = torch.Generator().manual_seed(_seed("metrics", B, T, C, joint_dim, b_div, family))
    m = torch.randn(B, T, C, generator=g)
    o = m + 0.6 * torch.randn(B, T, C, generator=g)
    if family == "scales":
        o[..., 0] *= 1e4
        if C > 1:
            o[..., 1] *= 1e-3
    elif family != "plain":
        raise ValueError(family)
    return o, m


def mse_ref(outputs, motions):
    """(exactly rounded float64 sum of the squares of the float32 differences, n_elems, relative gate n_elems x 2^-53)"""
    d = (outputs.float() - motions.float()).double().reshape(-1)
    return math.fsum((d * d).tolist()), d.numel(), d.numel() * 2.0 ** -53


def div_ref(outputs, b_div):
    """float64 [B // b_div]: 2 / (b (b - 1)) sum_{i<j} mean_e |o_i[e] - o_j[e]| per complete group of b_div consecutive clips"""
    o = outputs.double().reshape(outputs.shape[0], -1)
    vals = []
    for g in range(o.shape[0] // b_div):
        grp = o[g * b_div:(g + 1) * b_div]
        tot = 0.0
        for i in range(b_div - 1):
            tot += float((grp[i] - grp[i + 1:]).abs().sum())
        vals.append(tot / o.shape[1] * 2.0 / (b_div * (b_div - 1)))
    return np.asarray(vals, dtype=np.float64)


def div_gate(b_div):
    return b_div * 2.0 ** -24


def div_kernel_order(outputs, b_div, divisor=None, remainder=None, next_clip_cols=False):
    """metrics.hip's order on the CPU: per element column the inner sum over j in float32, one term at a time, everything behind in float64.
    Mutants: divisor (b_div^2 in place of b_div (b_div - 1)); remainder "own" (the incomplete last group gets a value of its own) or "merged"
    (its clips join the last complete group); next_clip_cols (the columns past clip_elems of the last 256-column chunk read the NEXT clip's
    first elements instead of zero; NaN behind the tensor)."""
    B = outputs.shape[0]
    o = outputs.float().reshape(B, -1)
    ce = o.shape[1]
    if next_clip_cols and ce % 256:
        pad = 256 - ce % 256
        flat = torch.cat((o.reshape(-1), torch.full((pad,), NAN)))
        o = torch.stack([flat[i * ce:i * ce + ce + pad] for i in range(B)])
    groups = [(g * b_div, (g + 1) * b_div) for g in range(B // b_div)]
    if remainder == "own" and B % b_div >= 2:
        groups.append((B - B % b_div, B))
    elif remainder == "merged" and B % b_div:
        groups[-1] = (groups[-1][0], B)
    vals = []
    for lo, hi in groups:
        grp, n = o[lo:hi], hi - lo
        tot = torch.zeros(o.shape[1], dtype=torch.float64)
        for i in range(n - 1):
            s = torch.zeros(o.shape[1])
            for j in range(i + 1, n):
                s += (grp[i] - grp[j]).abs()
            tot += s.double()
        vals.append(float(tot.sum()) / ce * 2.0 / (divisor or (n * (n - 1))))
    return np.asarray(vals, dtype=np.float64)


def div_check(got, ref, b_div, what="diversity"):
    """every group within relative b_div x 2^-24 of the float64 value; returns the largest error / gate"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: {got.shape[0]} groups, expected {ref.shape[0]}"
    rel = np.abs(got - ref) / ref
    assert np.all(rel <= div_gate(b_div)), f"{what}: relative error {rel.max():.3e} above b_div x 2^-24 = {div_gate(b_div):.3e}"
    return float(rel.max() / div_gate(b_div)) if len(rel) else 0.0


# ---- the encoder: latents against the packed layers evaluated on the host -------------------------------------------------------------------
ENC_CAL_CLIPS = 32


def encoder_gate(layers, x, n_poses, dim):
    """(packed_forward in float64 for every clip of x, calibration = max |packed_forward32 - packed_forward64| over the first ENC_CAL_CLIPS
    clips and both K orders): packed_forward32 is the same function in float32 with one accumulator per output (_mm)."""
    from metrics_ref import packed_forward
    assert x.shape[0] >= ENC_CAL_CLIPS
    ref = packed_forward(layers, x, n_poses, dim)
    xc = x[:ENC_CAL_CLIPS]
    cal = max(float((packed_forward(layers, xc, n_poses, dim, torch.float32, lambda a, w, r=r: _mm(a, w, r)).double() - ref[:ENC_CAL_CLIPS]).abs().max())
              for r in (False, True))
    return ref, cal
