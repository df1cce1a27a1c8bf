"""GPU tests (-m gpu) of the two kernels of the HuBERT encoder's bf16 precision mode as ops: dsh_op_gemm_bf16_pro (gemm_bf16_pro.hip) and
dsh_op_softmax_attention_bf16[_ragged] (audio_front.hip), against tests/hubert_bf16_ref.py.

Gates in the project's form, nothing fixed in advance.  Per element
    |out - ref64| <= [half a bf16 ulp for a bf16 store] + MARGIN x max |chain32 - ref64| + flip slack,
ref64 the documented chain in float64 (in front of the output store), chain32 the same chain in float32 with one accumulator per sum in both K
orders over a population of at least CAL_ROWS rows that contains the launch's own, flip slack = what ONE rounded operand that rounds the other
way can move the output by, computed from the fp64 operands: bf16_gates.flip_bound for the LayerNorm operand of the Linear (through GELU_LIP
where a GELU follows), hubert_bf16_ref.attn_flip_slack for the softmax weights.  The all-constant LayerNorm row adds
hubert_bf16_ref.const_row_slack (the rounding of the row mean, which torch's sum does not show).  Every case prints kernel / allowance."""
import ctypes as C

import pytest
import torch

import hubert_bf16_ref as ref
from bf16_gates import ATTN_FAMILIES, assert_rounded
from diffsheg_amd import _lib
from f32_gates import SENTINEL, assert_close_f32, two_pass

pytestmark = pytest.mark.gpu


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the Linear ------------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(128, 384), (256, 128), (1024, 128), (4096, 64), (1024, 3072)]
GEMM_MS = (1, 63, 64, 65, 129, 449)
LN_FAMILIES = ("plain", "off+50", "out300", "lowvar", "const")
GEMM_CASES = [(K, N, "f32", fam) for K, N in GEMM_SHAPES for fam in LN_FAMILIES] + [(K, N, "bf16", "plain") for K, N in GEMM_SHAPES]


def gemm_ms(K, N):
    return (65,) if (K, N) == (1024, 3072) else GEMM_MS


@pytest.mark.parametrize("K,N,kind,family", GEMM_CASES)
def test_gemm_bf16_pro(K, N, kind, family):
    L = _lib.lib()
    t = ref.gemm_case(K, N, kind, family, max(gemm_ms(K, N)))
    Xd = (t["X"] if kind == "bf16" else t["X"].float()).cuda()
    Wd, bd = t["W"].cuda(), t["b"].cuda()
    mom = None
    if kind == "f32" and K > 1024:          # rows wider than the moments launch takes: the caller's own two-pass moments
        mom = torch.cat(two_pass(t["X"].float()), 1).contiguous().cuda()
    worst = 0.0
    for out_bf16, act, res in ref.GEMM_COMBOS:
        ref64, slack = ref.gemm_gate(t, K, kind, family, act, res, own_moments=mom is None)
        for M in gemm_ms(K, N):
            out = torch.full((M + 2, N), SENTINEL, device="cuda", dtype=torch.bfloat16 if out_bf16 else torch.float32)
            if res:
                out[:M] = t["R"][:M].cuda()
            rc = L.dsh_op_gemm_bf16_pro(_stream(), Xd.data_ptr(), int(kind == "f32"), mom.data_ptr() if mom is not None else None, Wd.data_ptr(),
                                        bd.data_ptr(), out.data_ptr() if res else None, None if out_bf16 else out.data_ptr(),
                                        out.data_ptr() if out_bf16 else None, M, N, K, act, 0)
            _lib.check(rc, "dsh_op_gemm_bf16_pro")
            torch.cuda.synchronize()
            out = out.cpu()
            assert bool((out[M:] == torch.tensor(SENTINEL, dtype=out.dtype)).all()), "rows behind M were written"
            what = f"gemm_bf16_pro K={K} N={N} A={kind} {family} M={M} bf16_store={out_bf16} act={act} res={res}"
            fn = assert_rounded if out_bf16 else assert_close_f32
            worst = max(worst, fn(out[:M], ref64[:M], slack[:M], what, frames=M, nb=1))
    print(f"[measure] gemm_bf16_pro K={K} N={N} A={kind} {family}: worst |err| / allowance {worst:.3f}")


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_gemm_bf16_pro_tile_shapes_give_the_same_bits(kind):
    L = _lib.lib()
    K, N, M = 256, 384, 449
    g = torch.Generator().manual_seed(5)
    X = (torch.randn(M, K, generator=g) * 1.5 + 0.3)
    Xd = (X.bfloat16() if kind == "bf16" else X).cuda()
    Wd, bd = (torch.randn(N, K, generator=g) / 16).bfloat16().cuda(), torch.randn(N, generator=g).cuda()
    outs = []
    for tile in (1, 2):
        o = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        _lib.check(L.dsh_op_gemm_bf16_pro(_stream(), Xd.data_ptr(), int(kind == "f32"), None, Wd.data_ptr(), bd.data_ptr(), None, None, o.data_ptr(),
                                          M, N, K, 2, tile), "dsh_op_gemm_bf16_pro")
        outs.append(o)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    # rows do not depend on where they sit in M: rows 100 .. 199 alone
    o = torch.empty(100, N, device="cuda", dtype=torch.bfloat16)
    _lib.check(L.dsh_op_gemm_bf16_pro(_stream(), Xd[100:200].contiguous().data_ptr(), int(kind == "f32"), None, Wd.data_ptr(), bd.data_ptr(), None, None,
                                      o.data_ptr(), 100, N, K, 2, 0), "dsh_op_gemm_bf16_pro")
    torch.cuda.synchronize()
    assert torch.equal(o, outs[0][100:200])


def test_gemm_bf16_pro_refusals():
    L = _lib.lib()
    x = torch.zeros(64, 128, device="cuda")
    w = torch.zeros(128, 128, device="cuda", dtype=torch.bfloat16)
    b = torch.zeros(128, device="cuda")
    o = torch.full((64, 128), SENTINEL, device="cuda")
    call = lambda M, N, K, act=0, cf=True, cb=False, r=False: L.dsh_op_gemm_bf16_pro(
        _stream(), x.data_ptr(), 1, None, w.data_ptr(), b.data_ptr(), o.data_ptr() if r else None, o.data_ptr() if cf else None,
        o.data_ptr() if cb else None, M, N, K, act, 0)
    assert call(0, 128, 128) == -1
    assert call(64, 96, 128) == -1 and b"multiples of 64" in L.dsh_last_error()
    assert call(64, 128, 96) == -1
    assert call(64, 128, 128, act=1) == -1
    assert call(64, 128, 128, cf=False) == -1 and call(64, 128, 128, cb=True) == -1          # neither / both outputs
    assert call(64, 128, 128, cf=False, cb=True, r=True) == -1                               # a residual with the bf16 store
    torch.cuda.synchronize()
    assert bool((o == SENTINEL).all())
    assert call(64, 128, 128) == 0
    torch.cuda.synchronize()


# ---- the attention ---------------------------------------------------------------------------------------------------------------------
ATTN_MS = (1, 2, 31, 32, 33, 63, 64, 65, 151, 1000)
ATTN_BH = [(1, 2), (3, 2), (2, 16)]


def attn_ms(B, H):
    return tuple(M for M in ATTN_MS if M <= 65) if H == 16 else ATTN_MS


def attn_run(qkv, H, lens=None):
    L = _lib.lib()
    B, M, _ = qkv.shape
    q = qkv.cuda()
    out = torch.full((B * M + 2, H * 64), SENTINEL, device="cuda", dtype=torch.bfloat16)
    if lens is None:
        rc = L.dsh_op_softmax_attention_bf16(_stream(), q.data_ptr(), B, M, H, out.data_ptr())
    else:
        ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
        rc = L.dsh_op_softmax_attention_bf16_ragged(_stream(), q.data_ptr(), B, M, H, ld.data_ptr(), out.data_ptr())
    _lib.check(rc, "dsh_op_softmax_attention_bf16")
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[B * M:] == torch.tensor(SENTINEL, dtype=torch.bfloat16)).all()), "rows behind the output were written"
    return out[:B * M].reshape(B, M, H * 64)


@pytest.mark.parametrize("family", ATTN_FAMILIES)
@pytest.mark.parametrize("B,H", ATTN_BH)
def test_softmax_attention_bf16(B, H, family):
    worst = 0.0
    for M in attn_ms(B, H):
        qkv = ref.attn_qkv(B, M, H, family)
        r64, slack = ref.attn_gate(qkv, H)
        out = attn_run(qkv, H)
        worst = max(worst, assert_rounded(out.reshape(B * M, -1), r64.reshape(B * M, -1), slack.reshape(B * M, -1),
                                          f"softmax attention bf16 {family} B={B} H={H} M={M}", frames=M, nb=B))
    print(f"[measure] softmax attention bf16 {family} B={B} H={H}: worst |err| / allowance {worst:.3f}")


@pytest.mark.parametrize("M", [33, 65, 151])
def test_softmax_attention_bf16_ragged_rows_are_the_dense_rows(M):
    H = 2
    lens = [1, M, 32, M - 1, 33 if M > 33 else 2]
    B = len(lens)
    qkv = ref.attn_qkv(B, M, H, "plain")
    for b, n in enumerate(lens):
        qkv[b, n:] = float("nan")
    out = attn_run(qkv, H, lens)
    for b, n in enumerate(lens):
        alone = attn_run(qkv[b:b + 1, :n].contiguous(), H)
        assert torch.equal(out[b, :n], alone[0]), f"row {b} ({n} of {M} frames) differs from the dense call on it alone"
        assert bool((out[b, n:] == 0).all()), f"row {b}: frames behind its {n} are not zero"
    assert bool(torch.isfinite(out.float()).all())


def test_softmax_attention_bf16_batch_rows_are_bit_identical():
    B, M, H = 3, 151, 2
    qkv = ref.attn_qkv(B, M, H, "plain")
    full = attn_run(qkv, H)
    for b in range(B):
        assert torch.equal(attn_run(qkv[b:b + 1].contiguous(), H)[0], full[b])
