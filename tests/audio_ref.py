"""CPU oracle of the audio front (diffsheg_amd/csrc/audio_front.hip), written from the definitions and never from a kernel's output:
numpy float64 for the tables, plain torch for the evaluations (dtype-generic: float64 is the reference, float32 the calibration chain with
one accumulator per output and K ascending or descending, f32_gates._mm).

Mel spectrogram = librosa.feature.melspectrogram(y, sr=18000, hop_length=1200, n_mels=128)[..., :-1] of librosa 0.9.2, written out
(librosa itself is not needed and not used: this text is the specification):
  reflect-pad y by n_fft / 2 on both sides; frame j = the n_fft samples from hop j, j < len / hop (the last of the 1 + len / hop frames is
  dropped); periodic Hann window; power spectrum re^2 + im^2 at the n_fft / 2 + 1 bins; 128 Slaney filters from 0 to sr / 2 (mel = 3 f / 200
  below 1000 Hz, 15 + 27 ln(f / 1000) / ln 6.4 above; 130 points equally spaced in mel; triangles scaled by 2 / (m_{i+2} - m_i)), the
  filterbank rounded to fp32; no logarithm.

resample_poly = scipy.signal.resample_poly for given taps: zero-stuff, filter, decimate, taps centred, ceil(n up / down) outputs.
"""
import functools
import math

import numpy as np
import torch

from f32_gates import _mm

SR, N_FFT, HOP, N_MELS = 18000, 2048, 1200, 128


# ---- tables (numpy float64) -------------------------------------------------------------------------------------------------------------
def hann(n_fft=N_FFT):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)


@functools.lru_cache(maxsize=2)
def dft_table(n_fft=N_FFT):
    """[2 (n_fft / 2 + 1), n_fft] float64: window-folded cos rows, then sin rows; the angle reduced exactly as (k i) mod n_fft."""
    i = np.arange(n_fft, dtype=np.int64)
    a = 2.0 * np.pi * i.astype(np.float64) / n_fft
    cs, sn, w = np.cos(a), np.sin(a), hann(n_fft)
    r = (np.arange(n_fft // 2 + 1, dtype=np.int64)[:, None] * i[None, :]) % n_fft
    return np.concatenate((w[None, :] * cs[r], w[None, :] * sn[r]), 0)


def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f < 1000.0, 3.0 * f / 200.0, 15.0 + 27.0 * np.log(np.maximum(f, 1e-300) / 1000.0) / np.log(6.4))


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m < 15.0, 200.0 * m / 3.0, 1000.0 * np.exp(np.log(6.4) * (m - 15.0) / 27.0))


def mel_points(sr=SR, n_mels=N_MELS):
    lo, hi = float(hz_to_mel(0.0)), float(hz_to_mel(0.5 * sr))
    return mel_to_hz(lo + (hi - lo) * np.arange(n_mels + 2, dtype=np.float64) / (n_mels + 1))


@functools.lru_cache(maxsize=2)
def mel_filterbank(sr=SR, n_fft=N_FFT, n_mels=N_MELS):
    """[n_mels, n_fft / 2 + 1] float64 (the specification rounds it to fp32: .astype(np.float32))"""
    p = mel_points(sr, n_mels)
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * float(sr) / float(n_fft)
    lo = (f[None, :] - p[:-2, None]) / (p[1:-1, None] - p[:-2, None])
    up = (p[2:, None] - f[None, :]) / (p[2:, None] - p[1:-1, None])
    return np.maximum(0.0, np.minimum(lo, up)) * (2.0 / (p[2:, None] - p[:-2, None]))


# ---- mel spectrogram ------------------------------------------------------------------------------------------------------------------------
def num_frames(n, n_fft=N_FFT, hop=HOP):
    return n // hop if n >= n_fft // 2 + 1 and n >= hop else -1


def frames(y, n_fft=N_FFT, hop=HOP):
    """[len / hop, n_fft] rows of the reflect-padded signal (a torch tensor of any float dtype)"""
    n = y.shape[-1]
    assert num_frames(n, n_fft, hop) >= 1
    h = n_fft // 2
    yp = torch.cat((y[1:h + 1].flip(0), y, y[n - h - 1:n - 1].flip(0)))
    return torch.stack([yp[hop * j:hop * j + n_fft] for j in range(n // hop)])


def power_spectrum(y, dt, reverse=False):
    """[N, n_fft / 2 + 1] in dtype dt.  float64: the unrounded table; float32: the table as the library stores it, one accumulator per bin."""
    tab = dft_table(N_FFT)
    W = torch.from_numpy(tab) if dt == torch.float64 else torch.from_numpy(tab.astype(np.float32))
    s = _mm(frames(y.to(dt)), W, reverse)
    nb = N_FFT // 2 + 1
    return s[:, :nb] * s[:, :nb] + s[:, nb:] * s[:, nb:]


def melspectrogram(y, dt=torch.float64, reverse=False):
    """[len / 1200, 128] in dtype dt; the filterbank is the fp32-rounded one in both dtypes (it is part of the definition)"""
    fb = torch.from_numpy(mel_filterbank().astype(np.float32)).to(dt)
    return _mm(power_spectrum(y, dt, reverse), fb, reverse)


# ---- resample_poly ------------------------------------------------------------------------------------------------------------------------
def resample_taps(up, down):
    """scipy's default design in float64: firwin(2 h + 1, 1 / max(up, down), window=("kaiser", 5.0)) * up with h = 10 max(up, down):
    Kaiser(beta = 5) windowed sinc, scaled to unit gain at 0 Hz, then the gain `up`."""
    g = math.gcd(up, down)
    up, down = up // g, down // g
    r = max(up, down)
    half = 10 * r
    m = np.arange(-half, half + 1, dtype=np.float64)
    h = (1.0 / r) * np.sinc(m / r) * np.kaiser(2 * half + 1, 5.0)
    return h / h.sum() * up


def resample_len(n, up, down):
    return -(-n * up // down)


def resample_poly(x, up, down, taps, dt=np.float64):
    """x [n] -> [ceil(n up / down)] in dtype dt: y[j] = full[j down + half], full = (zero-stuffed x) * taps, the products added one tap at a
    time, taps ascending (the zero-stuffed samples add exact zeros)."""
    x = np.asarray(x, dtype=dt)
    taps = np.asarray(taps, dtype=dt)
    n, nt = x.shape[0], taps.shape[0]
    half = (nt - 1) // 2
    n_out = resample_len(n, up, down)
    xu = np.zeros(nt + n * up + down * n_out + nt, dtype=dt)          # nt zeros in front, zeros behind the signal
    xu[nt:nt + n * up:up] = x
    pos = nt + np.arange(n_out) * down + half
    acc = np.zeros(n_out, dtype=dt)
    for k in range(nt):
        acc = acc + taps[k] * xu[pos - k]
    return acc


# ---- softmax attention ----------------------------------------------------------------------------------------------------------------------
def softmax_attention(qkv, H, reverse=False):
    """qkv [B, M, 3 H 64] (q already scaled) -> [B, M, H 64] in qkv's dtype; float32: one accumulator per logit / output, channel and key order
    ascending (reverse: descending), torch's softmax."""
    B, M, _ = qkv.shape
    q, k, v = (qkv[:, :, i * H * 64:(i + 1) * H * 64].reshape(B, M, H, 64).permute(0, 2, 1, 3).reshape(B * H, M, 64) for i in range(3))
    if qkv.dtype != torch.float32:
        return (torch.softmax(q @ k.transpose(1, 2), -1) @ v).reshape(B, H, M, 64).permute(0, 2, 1, 3).reshape(B, M, H * 64)
    kt, o = k.transpose(1, 2).contiguous(), torch.zeros(B * H, M, 64)
    step = max(1, (1 << 21) // (M * M))                      # a few heads at a time: the logits of a block stay in the cache
    for i in range(0, B * H, step):
        s = torch.zeros(min(step, B * H - i), M, M)
        for c in (range(63, -1, -1) if reverse else range(64)):
            s.addcmul_(q[i:i + step, :, c:c + 1], kt[i:i + step, c:c + 1, :])
        p = torch.softmax(s, -1)
        for j in (range(M - 1, -1, -1) if reverse else range(M)):
            o[i:i + step].addcmul_(p[:, :, j:j + 1], v[i:i + step, j:j + 1, :])
    return o.reshape(B, H, M, 64).permute(0, 2, 1, 3).reshape(B, M, H * 64)
