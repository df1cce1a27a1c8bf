"""bf16 kernels on operands for which the answer is EXACT, so that no tolerance hides a wrong element (MI355X).

Integers in {-2 .. 2} (a quarter of the entries non-zero) for X and W, integer biases in [-4, 4], integer residuals |R| <= 64: every
partial sum is an exact fp32 integer in any order (sum |x w| < 2^24) and every result an exact bf16 integer (|y| < 256, asserted on
the reference), so the kernel's output must EQUAL the fp64 product - torch.equal, all rows, at row counts around every 32 / 128 / 256
block edge.  One-hot rows name a wrong element of the fragment / permutation order; a zero input with a bias grid sweeps the
activation epilogues; the folded LayerNorm is compared with the production fold (tl_pack_linear, as finalize() runs it), within the bound of its fp32 evaluation;
the attention kernels are given logits whose softmaxes are exactly uniform, so that y = the time mean of v, exactly.

Observed on an MI355X (each test prints its figure; the whole file takes 1.1 .. 1.3 s):
  every bit-equality holds as stated: token-per-lane Linears of both generations (plain, residual, hi / lo planes) at all eleven row
  counts, impulse rows, the GEMM at all nine shapes, and the attention kernels (no element needed the one-ulp fallback);
  GELU, fast polynomial of the token-per-lane epilogue: at most 9.0e-5 beyond the store's half ulp (allowed 1e-4; tl_common.h: 9.5e-5);
        erf form of the GEMM epilogue: 8.1e-8;
  SiLU, token-per-lane and GEMM epilogues: no element beyond the store's half ulp (allowed 2^-18 |y|) over the grid [-8, 8]; on integer
        pre-activations below -88 the GEMM's x / (1 + exp(-x)) returns -0 for a true -2.0e-37 (SILU_FLUSH below);
  folded LayerNorm: worst element at 0.94 (pro 1) and 0.84 (pro 3) of half an ulp + the bound (bound at most 1.3e-3 / 3.5e-3).
"""
import ctypes as C
import time

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import bf16_gates as G  # noqa: E402
from diffsheg_amd import _lib  # noqa: E402

DEV = "cuda:0"
ROWS = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 385)
ACT = {0: lambda v: v, 1: F.silu, 2: F.gelu}
# SiLU is evaluated as x / (1 + exp(-x)): below x = -88.7 the exponential overflows fp32 and the quotient is -0, where the true value is
# at most 89 e^-88.7 = 2.7e-37 (an integer pre-activation of -89 gives -2.0e-37); the hardware exp / rcp also flush denormals.  Results
# below 1e-36 may therefore come back as 0.
SILU_FLUSH = 1e-36


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module", autouse=True)
def _module_time():
    t0 = time.time()
    yield
    print(f"\n[bf16 exact] total time of this file {time.time() - t0:.1f} s")


def _ints(shape, g, top=2, density=0.25):
    v = torch.randint(1, top + 1, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    return (v * (torch.rand(shape, generator=g) < density)).float()


def _pad(t, mult=128):
    """Row buffers as the op tests allocate them: rows padded to a whole token block (the padding holds zeros)."""
    M = (t.shape[0] + mult - 1) // mult * mult
    out = torch.zeros(M, *t.shape[1:], dtype=t.dtype)
    out[:t.shape[0]] = t
    return out


def _tl(pro, X, W, b, R, cf, ct, Mv, act, K, gam=None, bet=None, film=None, frames=88, nb=1):
    """dsh_op_tl_linear on CPU tensors; returns (Cf, Ct) rows [:Mv] on the CPU."""
    N = W.shape[0]
    Xd, Wd, bd = _pad(X[:Mv]).to(DEV), W.to(DEV), b.to(DEV)
    Rd = None if R is None else _pad(R[:Mv]).to(DEV)
    M = Xd.shape[0]
    Cf = torch.full((M, N), float("nan"), device=DEV) if cf else None
    Ct = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16) if ct else None
    gd = (torch.ones(K) if gam is None else gam).to(DEV)
    be = (torch.zeros(K) if bet is None else bet).to(DEV)
    fd = None if film is None else film.to(DEV)
    _lib.check(_lib.lib().dsh_op_tl_linear(None, pro, _p(Xd), _p(Wd), _p(bd), _p(Rd), _p(Cf), _p(Ct), Mv, N, act, _p(gd), _p(be), _p(fd), frames, nb, K))
    torch.cuda.synchronize()
    return (None if Cf is None else Cf[:Mv].cpu()), (None if Ct is None else Ct[:Mv].cpu())


def _assert_equal(out, ref64, what):
    assert float(ref64.abs().max()) < 256, "the reference is not exactly representable in bf16: the operands of this test are wrong"
    if not torch.equal(out.double(), ref64):
        G.assert_close_f32(out, ref64, 0.0, what)          # raises with the worst element's position
        raise AssertionError(what)


def _set_gen(monkeypatch, gen, hilo=False):
    monkeypatch.setenv("DSH_TL2", "0" if gen == "1" else "1")
    monkeypatch.setenv("DSH_HILO", "1" if hilo else "0")


def _family(gen, hilo=False):
    return (10,) if gen == "1" else ((2,) if hilo else (0, 1))


# ---- integer operands: bit-equal ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def int_ops():
    g = torch.Generator().manual_seed(20)
    ops = {}
    for K, N in ((1024, 512), (512, 1024), (1024, 1024)):
        X, W = _ints((ROWS[-1], K), g), _ints((N, K), g)
        b = torch.randint(-4, 5, (N,), generator=g).float()
        R = torch.randint(-64, 65, (ROWS[-1], N), generator=g).float()
        ops[(K, N)] = (X.bfloat16(), W.bfloat16(), b, R, X.double() @ W.double().T + b.double())
    return ops


@pytest.mark.parametrize("mode", ["plain", "res", "res-hilo"])
@pytest.mark.parametrize("gen", ["2", "1"])
def test_tl_linear_integer_operands_are_bit_exact(int_ops, gen, mode, monkeypatch):
    """1024 -> 512, no prologue, no activation: bf16 out; with a residual fp32 + bf16 out, also on hi / lo planes (the lo plane of an
    integer is 0 and hi + lo exact).  Every row count around the 32 / 128 / 256 block edges, every element."""
    hilo = mode == "res-hilo"
    _set_gen(monkeypatch, gen, hilo)
    X, W, b, R, y = int_ops[(1024, 512)]
    for Mv in ROWS:
        ref = y[:Mv] + (R[:Mv].double() if mode != "plain" else 0)
        Cf, Ct = _tl(0, X, W, b, R if mode != "plain" else None, mode != "plain", True, Mv, 0, 1024)
        assert _lib.lib().dsh_debug_last_tl_variant() in _family(gen, hilo), "the launcher did not pick the family this test names"
        _assert_equal(Ct, ref, f"gen {gen} {mode} Mv {Mv} bf16 out")
        if Cf is not None:
            _assert_equal(Cf, ref, f"gen {gen} {mode} Mv {Mv} fp32 out")


@pytest.mark.parametrize("K,N,act", [(512, 1024, 2), (1024, 1024, 1)])
@pytest.mark.parametrize("gen", ["2", "1"])
def test_tl_linear_activation_of_an_exact_integer(int_ops, K, N, act, gen, monkeypatch):
    """ffn.linear1 + GELU and the SiLU instantiation: the pre-activation is an exact integer, the output act(integer) rounded to bf16."""
    _set_gen(monkeypatch, gen)
    X, W, b, _, y = int_ops[(K, N)]
    worst = 0.0
    for Mv in ROWS:
        _, Ct = _tl(0, X, W, b, None, False, True, Mv, act, K)
        assert _lib.lib().dsh_debug_last_tl_variant() in _family(gen)
        worst = max(worst, G.assert_rounded(Ct, ACT[act](y[:Mv]), 1e-4, f"gen {gen} act {act} Mv {Mv}"))
    print(f"[bf16 exact] tl_linear {K}->{N} act {act} gen {gen}: worst |out - act(integer)| / (0.5 ulp + 1e-4) = {worst:.3f}")


@pytest.mark.parametrize("K", [512, 1024])
@pytest.mark.parametrize("gen", ["2", "1"])
def test_tl_linear_impulse_rows_return_weight_columns(K, gen, monkeypatch):
    """Row m of X is one-hot at column (7 m + 3) % K (7 is coprime to K: K + 77 rows visit every column): out[m, :] must be
    bf16(W[:, k(m)] + b) exactly - a wrong element of the weight permutation or fragment order shows as the row and column it hits."""
    _set_gen(monkeypatch, gen)
    N, Mv = 512, K + 77
    g = torch.Generator().manual_seed(K)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    b = torch.randn(N, generator=g)
    k = (7 * torch.arange(Mv) + 3) % K
    X = torch.zeros(Mv, K).scatter_(1, k[:, None], 1.0).bfloat16()
    _, Ct = _tl(0, X, W, b, None, False, True, Mv, 0, K)
    want = (W.float().T[k] + b).bfloat16()                      # one fp32 addition, one rounding
    if not torch.equal(Ct, want):
        G.assert_close_f32(Ct, want.double(), 0.0, f"impulse K {K} gen {gen}")


def _bias_grid(N):
    special = torch.tensor([4.25, -4.25, 0.0, 8.0, -8.0, 1e-40, -1e-40, 2.0 ** -126, -2.0 ** -126, 1e-30, -1e-30, 4.25 + 2.0 ** -10, 4.25 - 2.0 ** -10])
    return torch.cat([special, torch.linspace(-8, 8, N - special.numel())])


def _activation_gate(out, bias, act, what):
    ref = ACT[act](bias.double()).expand(out.shape[0], -1)
    slack = 1e-4 if act == 2 else G.silu_hw(ref) + SILU_FLUSH
    ratio = G.assert_rounded(out, ref, slack, what)
    over = ((out.double() - ref).abs() - 0.5 * G.ulp_bf16(torch.maximum(out.double().abs(), ref.abs()))).clamp_min(0)
    if act == 1:
        over = torch.where(ref.abs() > SILU_FLUSH, over / ref.abs().clamp_min(SILU_FLUSH), torch.zeros_like(over))
    print(f"[bf16 exact] {what}: worst |out - ref| / allowance {ratio:.3f}; worst error beyond half an ulp "
          f"{float(over.max()):.3e}{' of |y|' if act == 1 else ' (absolute)'}")


@pytest.mark.parametrize("K,N,act", [(512, 1024, 2), (1024, 1024, 1)])
@pytest.mark.parametrize("gen", ["2", "1"])
def test_tl_linear_activation_sweep(K, N, act, gen, monkeypatch):
    """X = 0 and the bias a grid over [-8, 8] (with +-4.25, the clamp of the fast GELU, 0, denormals and +-8): out[:, n] = act(bias[n]).
    GELU against the exact erf form within half an ulp + 1e-4 (tl_common.h: 9.5e-5); SiLU within half an ulp + 2^-18 |y| for the
    hardware exp and rcp (an allowance, not a measurement: the observed maximum is printed)."""
    _set_gen(monkeypatch, gen)
    bias = _bias_grid(N)
    g = torch.Generator().manual_seed(1)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    _, Ct = _tl(0, torch.zeros(40, K).bfloat16(), W, bias, None, False, True, 40, act, K)
    _activation_gate(Ct, bias, act, f"tl_linear sweep {K}->{N} act {act} gen {gen}")


# ---- folded LayerNorm (second generation) ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,pro,act", [(512, 1536, 1, 0), (1024, 1024, 3, 1)])
def test_folded_layernorm_matches_the_fold_of_its_operands(K, N, pro, act, monkeypatch):
    """q|k|v behind a LayerNorm and feat_proj.1 behind the concat-LayerNorm (999 real columns) against
    y = rstd (x W'^T - mean c) + d built from W' = bf16(gamma W), c, d as the production packer folds them: the gate is the bound of the fp32
    evaluation of THAT expression on these operands (bf16_gates.tl_folded), not a fraction of the range.  (The unfolded LayerNorm
    differs from it by ~1e-2 here through the rounding of W'.)"""
    _set_gen(monkeypatch, "2")
    Mv, T, nb = 300, 64, 3
    kreal = 999 if pro == 3 else K
    t = G.tl_inputs(K, N, pro, False, Mv, T, nb)
    if pro == 3:
        t["X"][:, kreal:] = 0; t["W"][:, kreal:] = 0; t["gam"][kreal:] = 0; t["bet"][kreal:] = 0
    _, slack, ref = G.tl_folded(t, Mv, pro, act, kreal)
    if act == 1:
        slack = G.SILU_LIP * slack + G.silu_hw(ref)
    _, Ct = _tl(pro, t["X"], t["W"], t["b"], None, False, True, Mv, act, K, t["gam"], t["bet"], None, kreal if pro == 3 else T, 1)
    assert _lib.lib().dsh_debug_last_tl_variant() in (0, 1)
    ratio = G.assert_rounded(Ct, ref, slack, f"folded LN pro {pro}")
    print(f"[bf16 exact] folded LN pro {pro} {K}->{N}: worst |out - ref| / (0.5 ulp + bound) = {ratio:.3f}; bound max {float(slack.max()):.2e}")


def test_folded_layernorm_on_balanced_integer_rows(monkeypatch):
    """Rows of +-1 / 0 entries with as many +1 as -1: mean exactly 0, E[x^2] = n / 512 exactly; gamma = 1, beta = 0, integer W, so
    W' = W, d = b and y = rstd * integer + b, where only rstd (one hardware rsq), one product and one sum are inexact: 1e-6 relative
    on |rstd S| + |b| (fp32 output)."""
    _set_gen(monkeypatch, "2")
    K, N, Mv = 512, 512, 300
    g = torch.Generator().manual_seed(9)
    X = torch.zeros(Mv, K)
    for m in range(Mv):
        n = int(torch.randint(8, 200, (1,), generator=g))
        perm = torch.randperm(K, generator=g)
        X[m, perm[:n]] = 1.0; X[m, perm[n:2 * n]] = -1.0
    W = _ints((N, K), g)
    b = torch.randint(-4, 5, (N,), generator=g).float()
    Cf, _ = _tl(1, X.bfloat16(), W.bfloat16(), b, None, True, False, Mv, 0, K)
    rstd = 1 / torch.sqrt((X.double() ** 2).mean(-1, keepdim=True) + 1e-5)
    S = X.double() @ W.double().T
    ref = rstd * S + b.double()
    G.assert_close_f32(Cf, ref, 1e-6 * ((rstd * S).abs() + b.double().abs()), "folded LN, balanced integer rows")


# ---- tiled / weight-streaming GEMM ----------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(1, 2048, 2048), (4, 512, 2048), (5, 512, 2048), (16, 512, 2048), (17, 512, 2048),      # weight streaming up to 16 rows
               (16, 512, 2112),                                                                       # ... past its LDS limit: tiled
               (300, 8192, 1024),                                                                     # the 128 x 128 tile pick
               (64, 96, 64), (129, 200, 128)]                                                         # partial tiles, scalar epilogue


def _gemm(A, W, b, R, cf, ct, act):
    M, K = A.shape
    N = W.shape[0]
    Cf = torch.full((M, N), float("nan"), device=DEV) if cf else None
    Ct = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16) if ct else None
    _lib.check(_lib.lib().dsh_op_gemm(None, 1, _p(A), _p(W), _p(b), _p(R), _p(Cf), _p(Ct), M, N, K, act))
    torch.cuda.synchronize()
    return (None if Cf is None else Cf.cpu()), (None if Ct is None else Ct.cpu())


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_bf16_integer_operands_are_bit_exact(M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    A, W = _ints((M, K), g), _ints((N, K), g)
    b = torch.randint(-4, 5, (N,), generator=g).float()
    R = torch.randint(-64, 65, (M, N), generator=g).float()
    y = A.double() @ W.double().T + b.double()
    Ad, Wd, bd, Rd = A.bfloat16().to(DEV), W.bfloat16().to(DEV), b.to(DEV), R.to(DEV)
    for res in (False, True):
        ref = y + R.double() if res else y
        Cf, _ = _gemm(Ad, Wd, bd, Rd if res else None, True, False, 0)
        _assert_equal(Cf, ref, f"gemm {M}x{N}x{K} res {res} fp32 out")
        _, Ct = _gemm(Ad, Wd, bd, Rd if res else None, False, True, 0)
        _assert_equal(Ct, ref, f"gemm {M}x{N}x{K} res {res} bf16 out")
    for act in (1, 2):
        _, Ct = _gemm(Ad, Wd, bd, None, False, True, act)
        ref = ACT[act](y)
        G.assert_rounded(Ct, ref, 1e-4 if act == 2 else G.silu_hw(ref) + SILU_FLUSH, f"gemm {M}x{N}x{K} act {act}")


@pytest.mark.parametrize("M", [5, 129])
@pytest.mark.parametrize("act", [1, 2])
def test_gemm_bf16_activation_sweep(M, act):
    """Streaming (M = 5) and tiled (M = 129) kernels: A = 0, bias grid -> act(bias) in every row."""
    N, K = 1024, 128
    bias = _bias_grid(N)
    g = torch.Generator().manual_seed(2)
    W = torch.randn(N, K, generator=g).bfloat16().to(DEV)
    _, Ct = _gemm(torch.zeros(M, K, dtype=torch.bfloat16, device=DEV), W, bias.to(DEV), None, False, True, act)
    _activation_gate(Ct, bias, act, f"gemm sweep M {M} act {act}")


# ---- attention routing -------------------------------------------------------------------------------------------------------------------------
def _routing_qkv(nb, T, lens=None):
    """q constant over the channels of a frame, k constant over the frames of a channel: both softmaxes are exactly uniform
    (exp(0) = 1, sums T and 64: powers of two, so 1 / T and 1 / 64 are exact in bf16).  v = an integer per (clip, head, channel)
    plus +-1 alternating over the frames (zero sum over an even number of frames): y[b, t, :] = that integer, exactly."""
    D, H, hd = 512, 8, 64
    b_, t_, c_ = torch.arange(nb)[:, None, None], torch.arange(T)[None, :, None], torch.arange(D)[None, None, :]
    q = (((b_ * 5 + t_ * 3) % 17) - 8).float().expand(nb, T, D) / 4
    k = (((b_ * 7 + c_ * 3) % 23) - 11).float().expand(nb, T, D) / 4
    base = ((b_ * 37 + (c_ // hd) * 11 + (c_ % hd) * 3) % 201 - 100).float()
    v = base + (1.0 - 2.0 * (t_ % 2))
    qkv = torch.cat([q, k, v], dim=-1).bfloat16()
    if lens is not None:
        for b in range(nb):
            qkv[b, lens[b % len(lens)]:, D:] = float("nan")
    return qkv, base.expand(nb, T, D).double()


@pytest.mark.parametrize("nb", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("T", [32, 64])
def test_attention_routes_every_clip_head_and_channel(nb, T):
    qkv, want = _routing_qkv(nb, T)
    qd = qkv.to(DEV).contiguous()
    L = _lib.lib()
    outs = {}
    for name in ("bf16", "ragged-0", "ragged-1"):
        y = torch.full((nb, T, 512), float("nan"), device=DEV, dtype=torch.bfloat16)
        if name == "bf16":
            _lib.check(L.dsh_op_linear_attention_bf16(None, _p(qd), nb, T, 512, 64, _p(y)))
        else:
            _lib.check(L.dsh_op_linear_attention_ragged(None, 1, int(name[-1]), _p(qd), nb, T, 512, 64, _p(y), None, 0, None))
        torch.cuda.synchronize()
        outs[name] = y.cpu()
    for name, y in outs.items():
        if not torch.equal(y.double(), want):
            G.assert_close_f32(y.reshape(-1, 512), want.reshape(-1, 512), 0.0, f"attention {name} nb {nb} T {T}", frames=T, nb=nb)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("nb,doubled", [(1, False), (2, False), (3, False), (5, False), (8, False), (2, True), (6, True), (8, True)])
def test_ragged_attention_routes_every_clip_head_and_channel(nb, doubled, variant):
    """Clips of 8, 16 and 32 valid frames inside T = 64, NaN in the padded K / V rows; `doubled`: both CFG halves share the lengths."""
    T = 64
    nl = nb // 2 if doubled else nb
    lens = [(8, 16, 32)[i % 3] for i in range(nl)]
    qkv, want = _routing_qkv(nb, T, lens)
    qd = qkv.to(DEV).contiguous()
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    y = torch.full((nb, T, 512), float("nan"), device=DEV, dtype=torch.bfloat16)
    _lib.check(_lib.lib().dsh_op_linear_attention_ragged(None, 1, variant, _p(qd), nb, T, 512, 64, _p(y), _p(ld), nl, None))
    torch.cuda.synchronize()
    y = y.cpu()
    for b in range(nb):
        n = lens[b % nl]
        if not torch.equal(y[b, :n].double(), want[b, :n]):
            G.assert_close_f32(y[b, :n], want[b, :n], 0.0, f"ragged attention variant {variant} nb {nb} clip {b} ({n} of {T} frames)", frames=n, nb=1)
