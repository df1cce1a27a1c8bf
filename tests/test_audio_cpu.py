"""CPU tests of the audio front: the host-built tables of dsh_mel_* against the numpy float64 restatement (tests/audio_ref.py), that oracle
against independent implementations (torch.stft, scipy.signal), frame counts and refusals.  No GPU is touched: dsh_mel_create builds its
tables on the host and uploads nothing before the first dsh_mel_compute."""
import ctypes as C

import numpy as np
import pytest
import torch

import audio_ref
from diffsheg_amd import _lib, audio


@pytest.fixture(scope="module")
def mel():
    m = audio.MelSpectrogram()
    yield m
    m.close()


def test_mel_tables_equal_the_float64_restatement_rounded_to_fp32(mel):
    dft, fb = mel.tables()
    assert dft.shape == (2050, 2048) and fb.shape == (128, 1025)
    ref_dft = audio_ref.dft_table().astype(np.float32)
    ref_fb = audio_ref.mel_filterbank().astype(np.float32)
    assert np.array_equal(dft, ref_dft), f"{int((dft != ref_dft).sum())} DFT table entries differ"
    assert np.array_equal(fb, ref_fb), f"{int((fb != ref_fb).sum())} filterbank entries differ"


def test_mel_debug_tables_dims(mel):
    dims = (C.c_int32 * 3)()
    _lib.check(_lib.lib().dsh_mel_debug_tables(mel._h, dims, None, None))
    assert list(dims) == [1025, 2048, 128]


def test_dft_table_is_the_windowed_fourier_basis():
    tab = audio_ref.dft_table()
    i = np.arange(2048, dtype=np.float64)
    for k in (0, 1, 7, 512, 1023, 1024):
        w = audio_ref.hann()
        assert np.abs(tab[k] - w * np.cos(2 * np.pi * k * i / 2048)).max() < 1e-12
        assert np.abs(tab[1025 + k] - w * np.sin(2 * np.pi * k * i / 2048)).max() < 1e-12
    assert audio_ref.hann()[0] == 0.0 and abs(audio_ref.hann()[1024] - 1.0) < 1e-15          # periodic: the peak is sample n_fft / 2


def test_filterbank_shape_sign_peak_and_support(mel):
    _, fb = mel.tables()
    p = audio_ref.mel_points()
    assert p[0] == 0.0 and abs(p[-1] - 9000.0) < 1e-9 and np.all(np.diff(p) > 0)
    # the mel scale: linear below 1 kHz, 27 steps per factor 6.4 above
    assert abs(float(audio_ref.hz_to_mel(1000.0)) - 15.0) < 1e-12 and abs(float(audio_ref.hz_to_mel(6400.0)) - 42.0) < 1e-12
    assert abs(float(audio_ref.mel_to_hz(audio_ref.hz_to_mel(4321.0))) - 4321.0) < 1e-9
    peak = 2.0 / (p[2:] - p[:-2])                                   # the triangle's height at its centre m_{i+1}
    f = np.arange(1025) * 18000.0 / 2048.0
    assert np.all(fb >= 0.0)
    for i in range(128):
        nz = np.nonzero(fb[i])[0]
        assert nz.size >= 1, f"filter {i} has no bin at 18 kHz / 2048"
        assert np.all((f[nz] > p[i]) & (f[nz] < p[i + 2])), f"filter {i} reaches outside ({p[i]}, {p[i + 2]}) Hz"
        assert fb[i].max() <= np.float32(peak[i]) * (1 + 2.0 ** -23)
        # the bin nearest to the centre is within one bin spacing of the peak's slope
        d = np.abs(f - p[i + 1]).min()
        assert fb[i].max() >= peak[i] * (1.0 - d / min(p[i + 1] - p[i], p[i + 2] - p[i + 1])) * (1 - 1e-6)


@pytest.mark.parametrize("n,frames", [(1024, -1), (1025, -1), (1199, -1), (1200, 1), (2399, 1), (2400, 2), (1200 * 7 + 5, 7), (54000, 45)])
def test_mel_frame_counts(mel, n, frames):
    assert mel.num_frames(n) == frames == audio_ref.num_frames(n)


def test_oracle_power_spectrum_matches_torch_stft():
    g = torch.Generator().manual_seed(5)
    y = torch.randn(1200 * 7 + 5, generator=g, dtype=torch.float64)
    ours = audio_ref.power_spectrum(y, torch.float64)
    st = torch.stft(y, 2048, hop_length=1200, window=torch.hann_window(2048, periodic=True, dtype=torch.float64), center=True,
                    pad_mode="reflect", return_complex=True)
    ref = (st.real ** 2 + st.imag ** 2).T[:-1]                     # [frames, bins], the last frame dropped
    assert ours.shape == ref.shape == (7, 1025)
    assert float((ours - ref).abs().max()) <= 1e-10 * float(ref.max())


def test_oracle_float32_chain_is_close_to_float64():
    g = torch.Generator().manual_seed(6)
    y = torch.randn(2400, generator=g)
    ref = audio_ref.melspectrogram(y, torch.float64)
    for rev in (False, True):
        c = audio_ref.melspectrogram(y, torch.float32, rev).double()
        assert float((c - ref).abs().max()) <= 1e-4 * float(ref.max())
    assert float(audio_ref.melspectrogram(torch.zeros(1200), torch.float32).abs().max()) == 0.0


@pytest.mark.parametrize("up,down", [(9, 8), (2, 3)])
def test_resample_taps_and_restatement_match_scipy(up, down):
    signal = pytest.importorskip("scipy.signal")
    taps = audio.resample_taps(up, down)
    assert np.array_equal(taps, audio_ref.resample_taps(up, down))
    half = 10 * max(up, down)
    ref_taps = signal.firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    assert taps.shape == ref_taps.shape and np.abs(taps - ref_taps).max() <= 1e-14
    g = np.random.default_rng(3)
    for n in (1, 7, 8, 9, 1000):
        x = g.standard_normal(n)
        ours = audio_ref.resample_poly(x, up, down, taps)
        ref = signal.resample_poly(x, up, down)
        assert ours.shape == ref.shape == (audio_ref.resample_len(n, up, down),)
        assert np.abs(ours - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
        assert int(_lib.lib().dsh_resample_poly_len(n, up, down)) == ref.shape[0]
        given = signal.resample_poly(x, up, down, window=taps / up)           # caller-supplied taps: scipy multiplies them by `up`
        assert np.abs(ours - given).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def test_oracle_softmax_attention_float32_chain():
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(2, 33, 3 * 2 * 64, generator=g)
    qkv[:, :, :128] *= 0.125
    ref = audio_ref.softmax_attention(qkv.double(), 2)
    # against torch's own attention
    q, k, v = (qkv.double()[:, :, i * 128:(i + 1) * 128].reshape(2, 33, 2, 64).transpose(1, 2) for i in range(3))
    sdpa = torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=1.0).transpose(1, 2).reshape(2, 33, 128)
    assert float((ref - sdpa).abs().max()) < 1e-12
    for rev in (False, True):
        assert float((audio_ref.softmax_attention(qkv, 2, rev).double() - ref).abs().max()) < 1e-5


def test_normalize_wave():
    g = torch.Generator().manual_seed(8)
    w = torch.randn(5000, generator=g) * 3 + 2
    n = audio.normalize_wave(w)
    ref = (w.double() - w.double().mean()) / torch.sqrt(w.double().var(unbiased=False) + 1e-7)
    assert float((n.double() - ref).abs().max()) < 1e-5
