"""GPU tests (-m gpu) of the audio front (csrc/audio_front.hip): dsh_op_softmax_attention, dsh_mel_compute and dsh_op_resample_poly against
the CPU oracle tests/audio_ref.py.

Gates, in the project's form (bf16_gates.py / f32_gates.py): EVERY element |out - ref64| <= MARGIN x max |chain32 - ref64|, where ref64 is the
oracle in float64 and chain32 the same oracle in float32 with one accumulator per sum, taken in both summation orders; the calibration
population is drawn from the same input family and is never smaller than CAL_ROWS rows; no tolerance is fixed in advance.  Every test
prints kernel / calibration in front of its assertion.

The error of a DFT bin is relative to the frame's energy, not to the bin (2048 products of the size of the samples are added whatever the
result is), and so is that of a mel band; chain32 carries exactly that, so the allowance of a mel case is one number per input family.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import audio_ref
from diffsheg_amd import _lib, audio
from f32_gates import CAL_ROWS, MARGIN, SENTINEL, _seed, assert_close_f32

pytestmark = pytest.mark.gpu


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gate(chains, ref):
    """MARGIN x the largest |chain32 - ref64| over the given float32 evaluations"""
    return MARGIN * max(float((c.double() - ref).abs().max()) for c in chains)


# ---- softmax attention --------------------------------------------------------------------------------------------------------------------
ATTN_M = (1, 2, 31, 32, 33, 64, 65, 129, 1000)
ATTN_BH = ((1, 1), (3, 2), (2, 16))
ATTN_FAMILIES = ("plain", "big", "dom_last", "const")


def attn_rows(family, B, M, H, g):
    """qkv [B, M, 3 H 64] of one family; q carries its 1 / 8 already.
    plain: logits of unit variance; big: logits of +-60 and more (the online maximum has to carry them); dom_last: key M - 1, which lies in the
    last (for M % 32 != 0 partial) key tile, outweighs every other key by e^8 and more; const: rows of equal elements (logits 64 a_t b_s)."""
    x = torch.randn(B, M, 3, H, 64, generator=g)
    if family == "plain":
        x[:, :, 0] *= 0.125
    elif family == "big":
        x[:, :, 0] *= 2.5                        # logits ~ N(0, 20^2): the largest of a row is around +-60
    elif family == "dom_last":
        x[:, :, 0] *= 0.125
        x[:, :, 0, :, 0] = 2.0
        x[:, M - 1, 1, :, 0] = 6.0               # + 12 on the last key's logit, against 2 N(0, 1) on the others: it holds most of the
                                                 # weight, and the others still count far above the rounding of the sum
    elif family == "const":
        x[:, :, 0] = 0.125 * torch.randn(B, M, H, 1, generator=g)
        x[:, :, 1] = torch.randn(B, M, H, 1, generator=g)
        x[:, :, 2] = torch.randn(B, M, H, 1, generator=g)
    else:
        raise ValueError(family)
    return x.reshape(B, M, 3 * H * 64).contiguous()


@functools.lru_cache(maxsize=None)
def attn_extra_calibration(family, M):
    """max |chain32 - ref64| over CAL_ROWS and more query rows of the family at this M (single-head clips: heads do not interact)"""
    nb = max(1, -(-CAL_ROWS // M))
    qkv = attn_rows(family, nb, M, 1, torch.Generator().manual_seed(_seed("attn-cal", family, M)))
    ref = audio_ref.softmax_attention(qkv.double(), 1)
    return _gate([audio_ref.softmax_attention(qkv, 1, r) for r in (False, True)], ref)


def attn_calibration(family, M, qkv, H, ref):
    """MARGIN x max |chain32 - ref64| over the launch's own rows, both summation orders, and over further rows of the family where the launch
    has fewer than CAL_ROWS.  The launch's rows are part of the population, as in f32_gates.py: the error of a row grows with its largest
    logit (|s| 2^-24 per product), and in the families whose logit scale differs from row to row (const: 64 a_t b_s) the maximum of another
    draw of fewer rows is not the maximum of this one."""
    own = _gate([audio_ref.softmax_attention(qkv, H, r) for r in (False, True)], ref)
    return max(own, attn_extra_calibration(family, M)) if qkv.shape[0] * qkv.shape[1] * H < CAL_ROWS else own


def run_attention(qkv, H, tail_rows=2):
    B, M, _ = qkv.shape
    out = torch.full((B * M + tail_rows, H * 64), SENTINEL, device="cuda")
    _lib.check(_lib.lib().dsh_op_softmax_attention(_stream(), qkv.cuda().data_ptr(), B, M, H, out.data_ptr()), "dsh_op_softmax_attention")
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[B * M:] == SENTINEL).all()), "rows behind the output were written"
    return out[:B * M].reshape(B, M, H * 64)


@pytest.mark.parametrize("family", ATTN_FAMILIES)
@pytest.mark.parametrize("B,H", ATTN_BH)
@pytest.mark.parametrize("M", ATTN_M)
def test_softmax_attention(M, B, H, family):
    qkv = attn_rows(family, B, M, H, torch.Generator().manual_seed(_seed("attn", family, M, B, H)))
    ref = audio_ref.softmax_attention(qkv.double(), H)
    allow = attn_calibration(family, M, qkv, H, ref)
    out = run_attention(qkv, H)
    err = float((out.double() - ref).abs().max())
    print(f"[measure] softmax attention {family} M={M} B={B} H={H}: max err {err:.3e}, calibration {allow / MARGIN:.3e}, "
          f"kernel / calibration {err / max(allow / MARGIN, 1e-300):.2f}")
    assert_close_f32(out.reshape(B * M, H * 64), ref.reshape(B * M, H * 64), allow, f"softmax attention {family} M={M}", frames=M, nb=B)
    if B == 3:
        for b in range(B):
            alone = run_attention(qkv[b:b + 1], H)
            assert torch.equal(alone[0], out[b]), f"batch row {b} of B = 3 differs from the same row alone"


def test_softmax_attention_refusals():
    L = _lib.lib()
    x = torch.zeros(1, 4, 192, device="cuda")
    o = torch.zeros(1, 4, 64, device="cuda")
    assert L.dsh_op_softmax_attention(_stream(), None, 1, 4, 1, o.data_ptr()) == -1
    assert L.dsh_op_softmax_attention(_stream(), x.data_ptr(), 0, 4, 1, o.data_ptr()) == -1
    assert L.dsh_op_softmax_attention(_stream(), x.data_ptr(), 1, 0, 1, o.data_ptr()) == -1


# ---- mel spectrogram ------------------------------------------------------------------------------------------------------------------------
MEL_LENS = (1200, 2399, 2400, 1200 * 7 + 5, 54000)
MEL_FAMILIES = ("silence", "noise", "tone", "noise+dc")
CAL_LEN = CAL_ROWS * audio_ref.HOP


def mel_wave(family, n):
    """tone: amplitude 1 at exactly bin 150 of the 2048-point transform at 18 kHz (150 x 18000 / 2048 Hz): one bin holds everything, every
    other bin is round-off and leakage of the frame edges, the largest dynamic range a frame can have."""
    g = torch.Generator().manual_seed(_seed("mel", family))
    if family == "silence":
        return torch.zeros(n)
    if family == "noise":
        return 0.3 * torch.randn(n, generator=g)
    if family == "noise+dc":
        return 0.3 * torch.randn(n, generator=g) + 0.8
    if family == "tone":
        return torch.sin(2 * torch.pi * 150.0 * torch.arange(n, dtype=torch.float64) / 2048.0).float()
    raise ValueError(family)


@functools.lru_cache(maxsize=None)
def mel_calibration(family):
    """over the CAL_ROWS frames of a CAL_LEN-sample signal of the family; the launches get its first `len` samples"""
    y = mel_wave(family, CAL_LEN)
    ref = audio_ref.melspectrogram(y.double())
    return _gate([audio_ref.melspectrogram(y, torch.float32, r) for r in (False, True)], ref)


@pytest.fixture(scope="module")
def mel():
    m = audio.MelSpectrogram(device="cuda:0")
    yield m
    m.close()


@pytest.mark.parametrize("family", MEL_FAMILIES)
@pytest.mark.parametrize("n", MEL_LENS)
def test_mel(mel, n, family):
    y = mel_wave(family, CAL_LEN)[:n].contiguous()
    N = n // 1200
    out = mel(y.cuda())
    torch.cuda.synchronize()
    assert out.shape == (N, 128) and out.dtype == torch.float32
    out = out.cpu()
    if family == "silence":
        assert bool((out == 0).all()), "a silent input must give exact zeros"
        return
    ref = audio_ref.melspectrogram(y.double())
    allow = mel_calibration(family)
    err = float((out.double() - ref).abs().max())
    print(f"[measure] mel {family} len={n}: max err {err:.3e} (largest value {float(ref.max()):.3e}), calibration {allow / MARGIN:.3e}, "
          f"kernel / calibration {err / (allow / MARGIN):.2f}")
    assert_close_f32(out, ref, allow, f"mel {family} len={n}", frames=N, nb=1)


def test_mel_batch_rows_are_bit_identical_to_single_rows(mel):
    y = torch.stack([mel_wave(f, 1200 * 7 + 5) for f in ("noise", "tone", "noise+dc")])
    out = mel(y.cuda())
    for b in range(3):
        assert torch.equal(mel(y[b].cuda()), out[b]), f"batch row {b} of B = 3 differs from the same row alone"


def test_mel_refusals(mel):
    L = _lib.lib()
    w = torch.zeros(4096, device="cuda")
    o = torch.zeros(8, 128, device="cuda")
    assert L.dsh_mel_compute(mel._h, w.data_ptr(), 1, 1024, o.data_ptr()) == -1
    assert L.dsh_mel_compute(mel._h, w.data_ptr(), 1, 1199, o.data_ptr()) == -1
    assert L.dsh_mel_compute(mel._h, w.data_ptr(), 0, 2400, o.data_ptr()) == -1
    assert L.dsh_mel_compute(mel._h, None, 1, 2400, o.data_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((o == 0).all())
    with pytest.raises(ValueError):
        mel(w[:1024])


# ---- resample_poly --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resample_calibration(up, down):
    """fp32 against fp64 of the same sums over CAL_ROWS x 64 outputs of the same input family (unit normal samples)"""
    taps = audio.resample_taps(up, down)
    x = np.random.default_rng(_seed("resample-cal", up, down)).standard_normal(CAL_ROWS * 64 * down // up + 1)
    x32 = x.astype(np.float32)
    ref = audio_ref.resample_poly(x32, up, down, taps.astype(np.float32), np.float64)
    return MARGIN * float(np.abs(audio_ref.resample_poly(x32, up, down, taps.astype(np.float32), np.float32).astype(np.float64) - ref).max())


@pytest.mark.parametrize("up,down", [(9, 8), (2, 3)])
@pytest.mark.parametrize("n", (1, 7, 8, 9, 16000))
def test_resample_poly(n, up, down):
    taps = audio.resample_taps(up, down)
    x = torch.from_numpy(np.random.default_rng(_seed("resample", n, up, down)).standard_normal((2, n)).astype(np.float32))
    out = audio.resample_poly(x.cuda(), up, down)
    torch.cuda.synchronize()
    n_out = audio_ref.resample_len(n, up, down)
    assert out.shape == (2, n_out)
    ref = np.stack([audio_ref.resample_poly(x[b].numpy(), up, down, taps.astype(np.float32), np.float64) for b in range(2)])
    allow = resample_calibration(up, down)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    print(f"[measure] resample_poly {up}/{down} n={n}: max err {err:.3e}, calibration {allow / MARGIN:.3e}, "
          f"kernel / calibration {err / (allow / MARGIN):.2f}")
    assert_close_f32(out.cpu(), torch.from_numpy(ref), allow, f"resample_poly {up}/{down} n={n}")
    one = audio.resample_poly(x[1].cuda(), up, down)
    assert one.shape == (n_out,) and torch.equal(one, out[1])
