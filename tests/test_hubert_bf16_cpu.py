"""CPU tests of the HuBERT encoder's bf16 precision mode: the restatement tests/hubert_bf16_ref.py against the gates the GPU tests use (the
reference alone stays inside them, and each documented mutant is thrown out by at least one input family), the bf16 weight pack through the
host-only dsh_hubert_debug_packed, and the refusals of dsh_hubert_set_precision that need no device."""
import numpy as np
import pytest
import torch

import hubert_bf16_ref as ref
import hubert_ref
from bf16_gates import ATTN_FAMILIES, MARGIN, assert_rounded
from diffsheg_amd import _lib, audio
from f32_gates import assert_close_f32
from util import golden

SMALL = hubert_ref.SMALL
LN_FAMILIES = ("plain", "off+50", "out300", "lowvar", "const")
GEMM_K, GEMM_N, GEMM_ROWS = 256, 128, 129


def _fails(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


# ---- the restatement against the full-precision encoder ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [400, 719, 720, 16000])
def test_other_draws_of_the_chain_stay_inside_the_encoder_gate(n):
    """the GPU gate of test_gpu_hubert_bf16.py, with the float32 chain in the other K order and the float64 chain in the kernel's place"""
    fx = golden("hubert_small.npz")
    sd = hubert_ref.make_state_dict(SMALL, int(fx["sd_seed"]))
    x = hubert_ref.make_wave(n, int(dict(zip(fx["wave_lens"].tolist(), fx["wave_seeds"].tolist()))[n]))[None]
    full64 = torch.from_numpy(fx[f"out64_{n}"])
    stat = lambda y: ((y.double() - full64).abs().max().item(), (y.double() - full64).pow(2).mean().sqrt().item())
    gate = stat(ref.encode_bf16(sd, SMALL, x, torch.float32)[0])
    for what, y in (("float32 reversed", ref.encode_bf16(sd, SMALL, x, torch.float32, reverse=True)[0]),
                    ("float64", ref.encode_bf16(sd, SMALL, x, torch.float64)[0])):
        got = stat(y)
        print(f"[measure] n={n} {what}: max {got[0]:.3e} rms {got[1]:.3e}; gate chain max {gate[0]:.3e} rms {gate[1]:.3e}")
        assert got[0] <= MARGIN * gate[0] and got[1] <= MARGIN * gate[1]
    # bf16 layers are far from the fp32 encoder's own error: the mode is visible in the statistic the gate uses
    fp32 = stat(hubert_ref.encode(sd, SMALL, x, torch.float32)[0])
    assert gate[1] > 10 * fp32[1]


def test_encoder_mutants_move_the_output():
    """every mutant is wired through encode_bf16 and changes its output (a keyword that did nothing would make the op-level mutant tests below
    vacuous)"""
    sd = hubert_ref.make_state_dict(SMALL, 3)
    x = hubert_ref.make_wave(8000, 4)[None]
    base = ref.encode_bf16(sd, SMALL, x, torch.float64)
    for mut in (dict(ln="fold"), dict(store=ref.trunc), dict(l_rounded=True), dict(key_delta=-1), dict(gelu_before_bias=True)):
        assert float((ref.encode_bf16(sd, SMALL, x, torch.float64, **mut) - base).abs().max()) > 0, mut


# ---- the Linear's gate -------------------------------------------------------------------------------------------------------------------
def _gemm_check(t, y, kind, family, out_bf16, act, res):
    ref64, slack = ref.gemm_gate(t, GEMM_K, kind, family, act, res)
    fn = assert_rounded if out_bf16 else assert_close_f32
    M = GEMM_ROWS
    return fn((y.float().bfloat16() if out_bf16 else y.float())[:M], ref64[:M], slack[:M], f"{kind} {family}")


@pytest.mark.parametrize("kind,family", [("bf16", "plain")] + [("f32", f) for f in LN_FAMILIES])
def test_the_float32_chain_passes_the_linear_gate(kind, family):
    t = ref.gemm_case(GEMM_K, GEMM_N, kind, family, GEMM_ROWS)
    for out_bf16, act, res in ref.GEMM_COMBOS:
        for s in t["S32"]:
            _gemm_check(t, ref.gemm_epilogue(s, t, act, res), kind, family, out_bf16, act, res)


def test_fold_after_accumulate_layernorm_fails_on_a_large_row_mean():
    t = ref.gemm_case(GEMM_K, GEMM_N, "f32", "off+50", GEMM_ROWS)
    s = ref.linear(t["X"], t["W"], torch.zeros(GEMM_N), torch.float32, True, ln="fold")
    assert _fails(_gemm_check, t, ref.gemm_epilogue(s, t, 0, False), "f32", "off+50", False, 0, False)
    # ... and the normalise-first form of the same rows passes (test above); on centred rows the fold is harmless by comparison
    t0 = ref.gemm_case(GEMM_K, GEMM_N, "f32", "plain", GEMM_ROWS)
    e50 = (s.double() - t["S64"]).abs().max()
    e0 = (ref.linear(t0["X"], t0["W"], torch.zeros(GEMM_N), torch.float32, True, ln="fold").double() - t0["S64"]).abs().max()
    assert float(e50) > 5 * float(e0)


def test_truncating_store_fails_the_linear_gate():
    bad = 0
    for kind, family in [("bf16", "plain")] + [("f32", f) for f in LN_FAMILIES]:
        t = ref.gemm_case(GEMM_K, GEMM_N, kind, family, GEMM_ROWS)
        y = ref.gemm_epilogue(t["S32"][0], t, 0, False)
        ref64, slack = ref.gemm_gate(t, GEMM_K, kind, family, 0, False)
        bad += _fails(assert_rounded, ref.trunc(y, torch.float32).bfloat16()[:GEMM_ROWS], ref64[:GEMM_ROWS], slack[:GEMM_ROWS])
    assert bad >= 1


def test_gelu_before_the_bias_fails_the_linear_gate():
    bad = 0
    for family in LN_FAMILIES:
        t = ref.gemm_case(GEMM_K, GEMM_N, "f32", family, GEMM_ROWS)
        y = ref.linear(t["X"], t["W"], t["b"], torch.float32, True, act=2, gelu_before_bias=True)
        bad += _fails(_gemm_check, t, y, "f32", family, False, 2, False)
    assert bad >= 1


# ---- the attention's gate ----------------------------------------------------------------------------------------------------------------
ATTN_SHAPE = (2, 65, 2)          # B, M, H: three key tiles, the last one a single key


def _attn_check(qkv, H, y, lens=None):
    r64, slack = ref.attn_gate(qkv, H, lens)
    B, M, D = y.shape
    return assert_rounded(y.float().bfloat16().reshape(B * M, D), r64.reshape(B * M, D), slack.reshape(B * M, D), "attention", frames=M, nb=B)


@pytest.mark.parametrize("family", ATTN_FAMILIES)
def test_the_float32_chain_passes_the_attention_gate(family):
    B, M, H = ATTN_SHAPE
    qkv = ref.attn_qkv(B, M, H, family)
    for rev in (False, True):
        _attn_check(qkv, H, ref.attention(qkv, H, torch.float32, reverse=rev))
    lens = [33, 1]
    _attn_check(qkv, H, ref.attention(qkv, H, torch.float32, lens=lens), lens)


def _mutant_id(mutant):
    """str(mutant) with a function named instead of printed: its repr carries an address, which made the test's id differ from run to run"""
    return "{" + ", ".join(f"{k!r}: {getattr(v, '__name__', None) or repr(v)}" for k, v in mutant.items()) + "}"


@pytest.mark.parametrize("mutant", [dict(store=ref.trunc), dict(l_rounded=True), dict(key_delta=1), dict(key_delta=-1)], ids=_mutant_id)
def test_attention_mutants_fail_on_some_family(mutant):
    B, M, H = ATTN_SHAPE
    lens = [33, 40] if "key_delta" in mutant else None
    bad = []
    for family in ATTN_FAMILIES:
        qkv = ref.attn_qkv(B, M, H, family)
        if _fails(_attn_check, qkv, H, ref.attention(qkv, H, torch.float32, lens=lens, **mutant), lens):
            bad.append(family)
    print(f"[measure] attention mutant {mutant}: rejected on {bad}")
    assert bad


# ---- the weight pack -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handles():
    sd = hubert_ref.make_state_dict(SMALL, 1234)
    a = audio.HubertEncoder(SMALL, device=None, precision="bf16")
    b = audio.HubertEncoder(SMALL, device=None)
    a.load_tensors(sd)
    b.load_tensors(sd)
    yield a, b, sd
    a.close()
    b.close()


def test_bf16_pack_is_rne_of_the_float64_fold(handles):
    enc, f32, sd = handles
    assert enc.precision == "bf16" and f32.precision == "fp32"
    twice = 0
    for l in range(SMALL["layers"]):
        want = ref.layer_weights(sd, l)
        for kind in ("qkv", "out_proj", "ffn_in", "ffn_out"):
            W, b, c = enc.packed(kind, l)
            Ww, bw = want[kind]
            assert np.array_equal(W, Ww.float().numpy()), f"{kind} of layer {l}: not the one-step rounding of the fp64 fold"
            assert np.array_equal(W, torch.from_numpy(W).bfloat16().float().numpy())        # bf16 values
            assert np.array_equal(b, bw.numpy()) and not c.any()
            W32, b32, _ = f32.packed(kind, l)
            assert np.array_equal(b, b32)
            twice += int((torch.from_numpy(W32).bfloat16().float().numpy() != W).sum())
    print(f"[measure] weights that rounding through fp32 would have rounded the other way: {twice}")
    # everything in front of the layers is packed as the fp32 encoder packs it
    for kind, layer in [("conv", 0), ("conv", 6), ("feat_proj", 0), ("pos_conv", 0)]:
        for x, y in zip(enc.packed(kind, layer), f32.packed(kind, layer)):
            assert np.array_equal(x, y)


def test_rne64_rounds_once():
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8 + 2.0 ** -40), 0.0, 2.0 ** -130],
                     dtype=torch.float64)
    want = torch.tensor([1.0 + 2.0 ** -7, 1.0, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7), 0.0, 2.0 ** -130], dtype=torch.float64)
    assert torch.equal(ref.rne64(x), want)
    assert float(x[0].float().bfloat16()) == 1.0                       # the two-step rounding the pack must not take
    r = torch.randn(4096, dtype=torch.float64).float()
    assert torch.equal(ref.rne64(r), r.bfloat16().double())            # from fp32 there is only one step


def test_set_precision_refusals():
    L = _lib.lib()
    enc = audio.HubertEncoder(SMALL, device=None)
    for bad in (2, -1, 7):
        assert L.dsh_hubert_set_precision(enc._h, bad) == -1
        assert b"0 (fp32) or 1 (bf16)" in L.dsh_last_error()
    assert L.dsh_hubert_set_precision(None, 1) == -1
    assert L.dsh_hubert_set_precision(enc._h, 1) == 0 and L.dsh_hubert_set_precision(enc._h, 0) == 0
    enc.close()
    with pytest.raises(ValueError):
        audio.HubertEncoder(SMALL, device=None, precision="fp16")
    # intermediate a multiple of 32 but not of 64: fine in fp32, refused in bf16
    odd = dict(SMALL, intermediate=SMALL["intermediate"] + 32)
    audio.HubertEncoder(odd, device=None).close()
    with pytest.raises(_lib.DshError):
        audio.HubertEncoder(odd, device=None, precision="bf16")
