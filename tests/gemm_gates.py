"""Gates, the input builder and the case list for the generic GEMM (diffsheg_amd/csrc/gemm.hip: gemv_rows_kernel, gemm_nt_ksplit_kernel and the
five instantiations of gemm_nt_kernel behind one epilogue), derived from the arithmetic and never from a kernel's output (plain torch, CPU).
test_gemm_gates_cpu.py, gemm_worker.py and test_gpu_gemm.py build their operands here, so the CPU test checks the gates on the very operands
the GPU tests use.  The launches go through dsh_op_gemm_ex, which hands every field of the argument block to the caller.

  ref64    act(x W^T + b) + R[m % r], or act(x W^T + b + R[m % r]) with act_after_res, in float64.  bf16 cases round X and W to bf16 ONCE in the
           builder; the reference sees the rounded values, so the only bf16 rounding left is the store of a Ct output.
  chain32  the same expression in float32 with f32_gates._mm (one accumulator per output, K ascending), and with K descending.
  gate     EVERY element, |out - ref64| <= MARGIN x max |chain32 - ref64| over both orders and over max(M, CAL_ROWS) rows of the same draw.
           A bf16 Ct output adds the store's half ulp (assert_rounded with the allowance as slack).  No further slack.  The integer-operand
           cases (small integers, activation 0) have an exact answer in both dtypes and are compared bit for bit.
The kernels' summation orders are not copied into the gate.  test_gemm_gates_cpu.py emulates three of them (the K-split order, the GEMV's
lane-and-butterfly order, two products per accumulation step) and finds them at 0.06 .. 0.80 of the calibration at M 256, N 64, K 32 .. 2048,
so the reference alone stays well inside MARGIN.  No allowance exceeds accum_bound(|X|, |W|, K) (checked there on every case).

The worker puts GUARD rows of SENTINEL behind every output, SENTINEL into the columns N .. ld - 1 of every row when ld > N and into the other
half of the wide buffer of the column-slice form, and NaN behind every input (rows behind M, columns K .. lda - 1).

Kernel / calibration ratios (max |out - ref64|, a bf16 store's half ulp taken off, over max |chain32 - ref64|; printed by test_gpu_gemm.py in
front of every assertion), measured on an MI355X: the worst per kernel family and dtype over all cases and the seven latch settings
  GEMV     fp32 0.37 (5 x 3, K 32)        bf16 0.51 (16 x 17, K 64)
  K-split  fp32 1.13 (512 x 33, K 32)
  tiled    fp32 1.36 (896 x 100, K 64)    bf16 0.91 (513 x 60, K 128)    the same in all four tile shapes and the unswizzled form, which are
                                                                          bit-identical to each other on every tiled case
The gate allows MARGIN = 3.  No bf16 slack term was needed: the largest allowance any bf16 case uses is MARGIN x its calibration (plus the
half ulp of a Ct store), the bf16 matrix instruction's internal sum of 16 products stayed inside the fp32 calibration (0.91 at worst), and
every integer case came back bit-exact in every setting.
"""
import functools

import torch

from bf16_gates import accum_bound, assert_rounded, assert_store_is_rne, truncate_bf16, ulp_bf16  # noqa: F401  (re-exported for the tests)
from f32_gates import CAL_ROWS, MARGIN, SENTINEL, _ACTS, _mm, _seed, assert_close_f32, family_rows

F32, BF16 = 0, 1
DTYPE_NAME = {F32: "f32", BF16: "bf16"}
KTILE = {F32: 32, BF16: 64}              # elements of one 128-byte K tile
GUARD = 8                                # sentinel rows behind M of every output buffer


def _ints(shape, g, top=2, density=0.25):
    """small integers as test_gpu_bf16_exact._ints draws them: +-1 .. +-top at the given density, 0 elsewhere"""
    v = torch.randint(1, top + 1, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    return (v * (torch.rand(shape, generator=g) < density)).float()


# ---- one input builder --------------------------------------------------------------------------------------------------------------------
def inputs(M, N, K, dtype, act=0, act_after_res=0, res="none", out="both", lda_x=0, ldr_x=0, ldcf_x=0, ldct_x=0, ct_col=0, ints=False, family=None):
    """res: "none", "own" (a buffer of its own), "alias" (the residual IS the Cf buffer) or "mod<r>" (row m % r of an r-row table).
    out: "f" (Cf), "t" (Ct, the operand type) or "both".  *_x: extra width of a leading dimension; ct_col: column offset of Ct inside its
    ldct-wide buffer.  The draw depends on (M, N, K, dtype, ints) only: every epilogue form of one shape sees the same operands, which is
    what the bit-identity assertions between forms compare.  Always max(M, CAL_ROWS) rows; the launch gets the first M."""
    Mc = max(M, CAL_ROWS)
    g = torch.Generator().manual_seed(_seed("gemm", M, N, K, dtype, ints))
    if ints:
        X, W = _ints((Mc, K), g), _ints((N, K), g)
        b, R = _ints((N,), g, density=1.0), _ints((Mc, N), g, top=3, density=1.0)
        assert act == 0
    else:
        X = family_rows("plain", Mc, K, g)
        W, b, R = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g), torch.randn(Mc, N, generator=g)
    if dtype == BF16:
        X, W = X.bfloat16().float(), W.bfloat16().float()
    assert res in ("none", "own", "alias") or (res.startswith("mod") and int(res[3:]) > 0), res
    assert out in ("f", "t", "both") and (res != "alias" or out != "t"), (res, out)
    t = {"kind": "gemm", "M": M, "N": N, "K": K, "dtype": dtype, "act": act, "act_after_res": act_after_res, "res": res, "out": out, "ints": ints,
         "res_mod": int(res[3:]) if res.startswith("mod") else 0, "lda": K + lda_x, "ldcf": N + ldcf_x, "ldct": N + ldct_x, "ct_col": ct_col,
         "ldr": N + (ldcf_x if res == "alias" else ldr_x), "family": family, "X": X, "W": W, "b": b, "R": None if res == "none" else R}
    assert t["ct_col"] + N <= t["ldct"]
    return t


def epilogue(t, y, dt, bias=None, mod=None, swap_act=False):
    """bias -> activation -> + residual [-> activation] on the accumulators y, in dtype dt.  The keyword arguments are the mutants'."""
    y = y + (t["b"] if bias is None else bias).to(dt)
    act = _ACTS[t["act"]]
    if t["R"] is None:
        return act(y)
    r = t["res_mod"] if mod is None else mod
    m = torch.arange(y.shape[0])
    Rr = t["R"].to(dt)[m % r if r else m]
    return act(y + Rr) if bool(t["act_after_res"]) != swap_act else act(y) + Rr


def ref64(t, W=None, X=None, **kw):
    X, W = (t["X"] if X is None else X).double(), (t["W"] if W is None else W).double()
    return epilogue(t, X @ W.T, torch.float64, **kw)


def chain32(t, reverse=False):
    return epilogue(t, _mm(t["X"], t["W"], reverse), torch.float32)


def gate(t):
    """(ref64 over all calibration rows, allowance = MARGIN x calibration, calibration = max |chain32 - ref64| over both orders)"""
    if "_gate" not in t:
        ref = ref64(t)
        cal = max(float((chain32(t, r).double() - ref).abs().max()) for r in (False, True))
        t["_gate"] = (ref, MARGIN * cal, cal)
    return t["_gate"]


def outputs(t, y):
    """What a launch that computes the fp32 values y [>= M, N] stores: {"cf": fp32 or None, "ct": operand type or None}, M rows each"""
    y = y[:t["M"]].float()
    return {"cf": y.clone() if t["out"] != "t" else None, "ct": None if t["out"] == "f" else (y.bfloat16() if t["dtype"] == BF16 else y.clone())}


def check(t, outs, what=None, extra=0.0):
    """Gate the outputs of one launch ({"cf", "ct"}: [M, N] each or None) on every element.  Returns the worst |diff| / allowance."""
    what = what or t.get("name", "gemm")
    M = t["M"]
    ref, allow, cal = gate(t)
    ref = ref[:M]
    cf, ct = outs["cf"], outs["ct"]
    assert (cf is None) == (t["out"] == "t") and (ct is None) == (t["out"] == "f"), what
    worst = 0.0
    if t["ints"]:
        for k, o in (("Cf", cf), ("Ct", ct)):
            if o is not None:
                bad = o.double() != ref
                assert not bool(bad.any()), f"{what} {k}: {int(bad.sum())} of {bad.numel()} elements differ from the exact integer result; first {bad.nonzero()[0].tolist()}"
        return 0.0
    if cf is not None:
        worst = max(worst, assert_close_f32(cf, ref, allow + extra, f"{what} Cf"))
    if ct is not None and t["dtype"] == BF16:
        worst = max(worst, assert_rounded(ct, ref, allow + extra, f"{what} Ct"))
    elif ct is not None:
        worst = max(worst, assert_close_f32(ct, ref, allow + extra, f"{what} Ct"))
    if cf is not None and ct is not None:
        if t["dtype"] == BF16:
            assert_store_is_rne(ct, cf, f"{what}: Ct beside Cf")
        else:
            assert torch.equal(ct, cf), f"{what}: the fp32 Ct differs from Cf"
    return worst


def ratio(t, outs):
    """kernel / calibration without asserting: max |out - ref64| (a bf16 store's half ulp taken off) over the calibration maximum"""
    ref, allow, cal = gate(t)
    ref = ref[:t["M"]]
    if outs["cf"] is not None:
        err = (outs["cf"].double() - ref).abs()
    else:
        err = (outs["ct"].double() - ref).abs()
        if t["dtype"] == BF16:
            err = (err - 0.5 * ulp_bf16(torch.maximum(outs["ct"].double().abs(), ref.abs()))).clamp_min(0.0)
    return (float(err.max()) / cal if cal > 0 else float(err.max())), cal


# ---- emulated summation orders (fp32; the CPU test runs them through the gate) ------------------------------------------------------------
def _cols_mm(X, W, cols):
    if len(cols) == 0:
        return torch.zeros(X.shape[0], W.shape[0])
    cols = torch.as_tensor(cols)
    return _mm(X[:, cols].contiguous(), W[:, cols].contiguous(), False)


def emulate_ksplit(t, drop_tile=None):
    """gemm_nt_ksplit_kernel: wave w of eight adds the K tiles w, w + 8, ... in ascending k, wave 0 adds the partial sums ((w0 + w1) + w2) + ..."""
    kt = KTILE[t["dtype"]]
    nk = t["K"] // kt
    acc = None
    for w in range(8):
        cols = [k for tile in range(w, nk, 8) if tile != drop_tile for k in range(tile * kt, (tile + 1) * kt)]
        part = _cols_mm(t["X"], t["W"], cols)
        acc = part if acc is None else acc + part
    return epilogue(t, acc, torch.float32)


def gemv_steps(t):
    epl = 16 // (4 if t["dtype"] == F32 else 2)
    return (t["K"] + 64 * epl - 1) // (64 * epl), epl


def emulate_gemv(t, drop_last_step=False):
    """gemv_rows_kernel: lane l of 64 adds its 16-byte pieces (4 fp32 / 8 bf16 elements) of every 64-lane step in ascending k, then a
    butterfly over the lanes (xor 32, 16, .. 1)."""
    nsteps, epl = gemv_steps(t)
    K = t["K"]
    lanes = []
    for lane in range(64):
        cols = [k for st in range(nsteps - (1 if drop_last_step else 0)) for k in range((st * 64 + lane) * epl, (st * 64 + lane + 1) * epl) if k < K]
        lanes.append(_cols_mm(t["X"], t["W"], cols))
    v = torch.stack(lanes)                                   # [64, Mc, N]
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[idx ^ o]
    return epilogue(t, v[0], torch.float32)


def emulate_pairs(t):
    """two products per accumulation step (the fp32 matrix instruction's K = 2): acc += x0 w0 + x1 w1, K ascending"""
    X, wt = t["X"], t["W"].T.contiguous()
    acc = torch.zeros(X.shape[0], wt.shape[1])
    for k in range(0, t["K"], 2):
        acc += X[:, k:k + 1] * wt[k][None, :] + X[:, k + 1:k + 2] * wt[k + 1][None, :]
    return epilogue(t, acc, torch.float32)


# ---- which kernel a launch takes (the dispatch rules of launch_gemm_t, restated) ----------------------------------------------------------
SETTINGS = {"default": {}, "tile0": {"DSH_GEMM_TILE": "0"}, "tile2": {"DSH_GEMM_TILE": "2"}, "tile4": {"DSH_GEMM_TILE": "4"},
            "variant0": {"DSH_GEMM_VARIANT": "0"}, "gemv0": {"DSH_GEMV": "0"}, "ksplit0": {"DSH_GEMM_KSPLIT": "0"}}
TILE_BM = {0: 128, 1: 128, 2: 64, 3: 64, 4: 128}            # rows of the tile per pick (4: the unswizzled 128 x 128 form)
COUNTER = {"gemv": "gemv", "ksplit": "gemm_f32_fewrow", "tiled": {F32: "gemm_f32_tiled", BF16: "gemm_bf16_tiled"}}


def expected_launch(M, N, K, dtype, env=None):
    """(family, tile pick or None) of a launch under the environment of one latch setting"""
    env = env or {}
    if int(env.get("DSH_GEMV", 1)) and M <= 16 and (4 if M <= 4 else 16) * K * 4 <= 128 * 1024:
        return "gemv", None
    if dtype == F32 and M <= int(env.get("DSH_GEMM_KSPLIT", 512)):
        return "ksplit", None
    if int(env.get("DSH_GEMM_VARIANT", 1)) == 0:
        return "tiled", 4
    sel = int(env.get("DSH_GEMM_TILE", 1))
    if sel == 0:
        return "tiled", 0
    if 2 <= sel <= 4:
        return "tiled", sel - 1
    return "tiled", 0 if dtype == BF16 and sel == 1 and M <= 2048 and N >= 8192 and K >= 1024 else 2


def expected_counts(t, env=None):
    """the launch counters one launch of the case leaves: {counter name: 1} and the tile pick (None: not a tiled launch)"""
    fam, pick = expected_launch(t["M"], t["N"], t["K"], t["dtype"], env)
    name = COUNTER[fam] if fam != "tiled" else COUNTER[fam][t["dtype"]]
    return {n: int(n == name) for n in ("gemv", "gemm_f32_fewrow", "gemm_f32_tiled", "gemm_bf16_tiled")}, pick


# ---- the case list (shared by the CPU test, the GPU test and the worker) -------------------------------------------------------------------
GEMV_M, GEMV_N = (1, 4, 5, 16), (1, 3, 4, 15, 16, 17, 100)
GEMV_K = {F32: (32, 256, 288, 512, 544, 2048), BF16: (64, 512, 576, 1024, 1088, 2048)}
KS_M, KS_N, KS_K = (17, 31, 32, 33, 512), (4, 30, 33, 100), (32, 224, 256, 288, 544)
TILED_M = {F32: (513, 575, 577), BF16: (513, 575, 577, 17, 63, 64, 65, 129, 449)}
TILED_N = (4, 60, 64, 68, 100, 132)
NTM_M = (448, 449, 512, 513, 896, 897, 1025)                # 7 | 8 | 8 | 9 tiles of 64 rows, 7 | 8 | 9 tiles of 128 rows
FORM_SHAPES = {("gemv", F32): (5, 100, 512), ("gemv", BF16): (5, 100, 512), ("ksplit", F32): (40, 100, 288),
               ("tiled", F32): (577, 100, 96), ("tiled", BF16): (130, 100, 192)}
_RES, _OUT = ("none", "own", "alias", "mod11"), ("both", "f", "t")
# epilogue forms: name -> builder keywords (N is the case's width; a callable gets it)
FORMS = {
    "act0": {}, "act1": {"act": 1}, "act2": {"act": 2},
    "res-own": {"act": 1, "res": "own"}, "res-alias": {"act": 1, "res": "alias"}, "res-mod11": {"act": 1, "res": "mod11"}, "res-mod3": {"act": 2, "res": "mod3"},
    "after-res": {"act": 1, "act_after_res": 1, "res": "own"}, "after-res-mod3": {"act": 1, "act_after_res": 1, "res": "mod3"},
    "out-f": {"out": "f", "res": "own"}, "out-t": {"out": "t", "res": "own"},
    "ldcf+4": {"res": "own", "ldcf_x": 4}, "ldcf+3": {"res": "own", "ldcf_x": 3}, "ldcf+4-alias": {"res": "alias", "ldcf_x": 4}, "ldcf+3-alias": {"res": "alias", "ldcf_x": 3},
    "ct-slice": lambda N: {"res": "own", "ldct_x": N, "ct_col": N},
    "lda+tile": lambda N: {"res": "own", "lda_x": "tile"},
    "ldr+4": {"res": "own", "ldr_x": 4},
}
INT_FORMS = ("act0", "ldcf+4", "ldcf+3", "ldcf+4-alias", "ldcf+3-alias", "ct-slice", "lda+tile", "ldr+4", "out-f", "out-t")
INT_EXTRA = {"int-res-alias": {"res": "alias"}, "int-res-mod11": {"res": "mod11"}, "int-res-mod3": {"res": "mod3"}}


def _grid_kw(j):
    """the epilogue of a grid case alternates with its shape: activation, residual and outputs"""
    res = _RES[j % 4]
    out = _OUT[(j // 2) % 3]
    return {"act": j % 3, "res": res, "out": "both" if res == "alias" and out == "t" else out, "act_after_res": int(j % 5 == 0 and res != "none")}


def _cases():
    c = {}

    def add(name, M, N, K, dt, family, **kw):
        if kw.get("lda_x") == "tile":
            kw["lda_x"] = KTILE[dt]
        c[f"{name}-{DTYPE_NAME[dt]}-{M}x{N}x{K}"] = dict(kw, M=M, N=N, K=K, dtype=dt, family=family)

    for dt in (F32, BF16):
        kt = KTILE[dt]
        # GEMV: the cross product thinned to a third; its LDS limits in full (the two shapes past a limit leave the GEMV)
        for im, M in enumerate(GEMV_M):
            for i_n, N in enumerate(GEMV_N):
                for ik, K in enumerate(GEMV_K[dt]):
                    j = im + i_n + ik
                    if (j + dt) % 3 == 0:
                        add("gemv", M, N, K, dt, "gemv", **_grid_kw(j))
        off = "ksplit" if dt == F32 else "tiled"
        for j, (M, N, K, fam) in enumerate(((4, 16, 8192, "gemv"), (4, 16, 8192 + kt, off), (5, 16, 2048, "gemv"), (16, 16, 2048, "gemv"), (16, 16, 2048 + kt, off))):
            add("gemv-limit", M, N, K, dt, fam, **_grid_kw(j))
        # tiled at the default pick (64 x 64; the one 128 x 128-rule shape below)
        for im, M in enumerate(TILED_M[dt]):
            for i_n, N in enumerate(TILED_N):
                for ik, K in enumerate((kt, 2 * kt, 3 * kt, 1024)):
                    j = im + i_n + ik
                    if (j + dt) % 3 == 0:
                        add("tiled", M, N, K, dt, "tiled", **_grid_kw(j))
        # 7, 8 and 9 row tiles of either tile height (fp32 at 512 rows or fewer is tiled under DSH_GEMM_KSPLIT=0 only)
        for j, M in enumerate(NTM_M):
            add("ntm", M, 100, 2 * kt, dt, "ksplit" if dt == F32 and M <= 512 else "tiled", **_grid_kw(j))
    add("tiled-128rule", 300, 8192, 1024, BF16, "tiled", act=0, res="none", out="t")
    # K-split (fp32): fewer, exactly and one more K tile than waves; N % 32 and N % 4
    for im, M in enumerate(KS_M):
        for i_n, N in enumerate(KS_N):
            for ik, K in enumerate(KS_K):
                j = im + i_n + ik
                if j % 2 == 0:
                    add("ksplit", M, N, K, F32, "ksplit", **_grid_kw(j))
    # every epilogue form at one shape per kernel family and dtype, N = 100 (the last 32-column tile holds one 4-column group) and N = 104
    # (two groups: both halves of the wave store), plus the exact integer versions
    for (fam, dt), (M, N0, K) in FORM_SHAPES.items():
        for N in (N0, N0 + 4):
            for form, kw in FORMS.items():
                add(f"form-{form}", M, N, K, dt, fam, **(kw(N) if callable(kw) else kw))
            for form in INT_FORMS:
                kw = FORMS[form]
                add(f"int-{form}", M, N, K, dt, fam, ints=True, **(kw(N) if callable(kw) else kw))
            for form, kw in INT_EXTRA.items():
                add(form, M, N, K, dt, fam, ints=True, **kw)
    return c


CASES = _cases()
_BIG = ("tiled-128rule-bf16-300x8192x1024",)


@functools.lru_cache(maxsize=8)          # (forms of one shape run next to each other; the gate of a case is computed once per process)
def case(name):
    t = inputs(**CASES[name])
    t["name"] = name
    return t


def case_names(prefix=""):
    return [n for n in CASES if n.startswith(prefix)]


def sibling(name, form_a, form_b):
    """the name of the same shape's case with another epilogue form"""
    assert f"form-{form_a}-" in name or f"int-{form_a}-" in name, (name, form_a)
    return name.replace(f"-{form_a}-", f"-{form_b}-", 1)
