"""Audio front on the device (csrc/audio_front.hip): what the reference's ``test_custom_aud`` (trainers/ddpm_show_trainer.py:944-1100,
ddpm_beat_trainer.py:1123-1340) computes from a speech signal in front of the sampler.

    mel   = MelSpectrogram()(wave18k)            # [N, 128], N = len // 1200: librosa.feature.melspectrogram(..)[..., :-1]
    w18k  = resample_poly(wave16k, 9, 8)         # scipy.signal.resample_poly semantics

Everything stays on the device; the kernels are HIP (there is no torch fallback).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib

MEL_SR, MEL_N_FFT, MEL_HOP, MEL_N_MELS = 18000, 2048, 1200, 128      # the reference's melspectrogram call


def normalize_wave(w: torch.Tensor) -> torch.Tensor:
    """``(w - mean) / sqrt(var + 1e-7)`` with the population variance over the whole utterance: what the reference's ``Wav2Vec2Processor``
    call does in front of HuBERT (before any chunking)."""
    w = w.to(torch.float32)
    return (w - w.mean()) / torch.sqrt(w.var(unbiased=False) + 1e-7)


def resample_taps(up: int, down: int) -> np.ndarray:
    """The FIR of ``scipy.signal.resample_poly``'s default, designed in float64: Kaiser (beta = 5) windowed sinc of half-length
    ``10 max(up, down)`` and cutoff ``1 / max(up, down)``, unit gain at 0 Hz times ``up`` (``up`` / ``down`` reduced by their gcd)."""
    g = math.gcd(int(up), int(down))
    up, down = int(up) // g, int(down) // g
    r = max(up, down)
    half = 10 * r
    m = np.arange(-half, half + 1, dtype=np.float64)
    h = (1.0 / r) * np.sinc(m / r) * np.kaiser(2 * half + 1, 5.0)
    return h / h.sum() * up


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def resample_poly(x: torch.Tensor, up: int, down: int, taps=None) -> torch.Tensor:
    """``scipy.signal.resample_poly(x, up, down)`` along the last axis of ``x [n]`` or ``[B, n]`` (device fp32) on the device.  ``taps``
    (odd length, gain included; default :func:`resample_taps`) are rounded to fp32.  The reference resamples with resampy's
    ``kaiser_best`` filter instead: same band, other taps."""
    if not x.is_cuda:
        raise _lib.DshError("resample_poly runs on the GPU: there is no CPU fallback")
    g = math.gcd(int(up), int(down))
    up, down = int(up) // g, int(down) // g
    x2 = x.to(torch.float32).reshape(-1, x.shape[-1]).contiguous()
    if up == down:
        return x2.clone().reshape(x.shape)
    h = resample_taps(up, down) if taps is None else np.asarray(taps, dtype=np.float64)
    if h.ndim != 1 or h.shape[0] % 2 != 1:
        raise ValueError("resample_poly takes an odd number of taps")
    B, n = int(x2.shape[0]), int(x2.shape[1])
    L = _lib.lib()
    n_out = int(L.dsh_resample_poly_len(n, up, down))
    taps_dev = torch.from_numpy(h.astype(np.float32)).to(x2.device)
    y = torch.empty(B, n_out, device=x2.device, dtype=torch.float32)
    _lib.check(L.dsh_op_resample_poly(_stream(x2.device), x2.data_ptr(), B, n, up, down, taps_dev.data_ptr(), int(h.shape[0]), y.data_ptr()),
               "dsh_op_resample_poly")
    return y.reshape(tuple(x.shape[:-1]) + (n_out,))


class MelSpectrogram:
    """``librosa.feature.melspectrogram(y, sr=18000, hop_length=1200, n_mels=128)[..., :-1]`` transposed to frames-first, as the reference
    feeds it to the model: ``mel = MelSpectrogram()(wave)`` for ``wave [len]`` or ``[B, len]`` gives ``[len // 1200, 128]`` or
    ``[B, len // 1200, 128]`` fp32 on the device (power spectrogram, no logarithm).  Needs ``len >= 1200``."""

    def __init__(self, sr: int = MEL_SR, n_fft: int = MEL_N_FFT, hop: int = MEL_HOP, n_mels: int = MEL_N_MELS, device=None):
        self.sr, self.n_fft, self.hop, self.n_mels = int(sr), int(n_fft), int(hop), int(n_mels)
        self._lib = _lib.lib()
        self.device = torch.device(device) if device is not None else None
        stream = 0
        if self.device is not None:
            torch.cuda.set_device(self.device)
            self._stream = torch.cuda.current_stream(self.device)
            stream = self._stream.cuda_stream
        self._h = C.c_void_p()
        _lib.check(self._lib.dsh_mel_create(self.sr, self.n_fft, self.hop, self.n_mels, C.c_void_p(stream), C.byref(self._h)), "dsh_mel_create")

    def num_frames(self, n: int) -> int:
        return int(self._lib.dsh_mel_num_frames(self._h, int(n)))

    def tables(self):
        """Host only: ``(dft [2 (n_fft / 2 + 1), n_fft], fb [n_mels, n_fft / 2 + 1])`` float32, as the device holds them."""
        nb = self.n_fft // 2 + 1
        dft = np.empty((2 * nb, self.n_fft), dtype=np.float32)
        fb = np.empty((self.n_mels, nb), dtype=np.float32)
        _lib.check(self._lib.dsh_mel_debug_tables(self._h, None, dft.ctypes.data_as(C.c_void_p), fb.ctypes.data_as(C.c_void_p)),
                   "dsh_mel_debug_tables")
        return dft, fb

    def __call__(self, wave: torch.Tensor) -> torch.Tensor:
        if self.device is None:
            raise _lib.DshError("MelSpectrogram was created without a device: there is no CPU fallback")
        if wave.dim() not in (1, 2):
            raise ValueError(f"MelSpectrogram takes [len] or [B, len], got {tuple(wave.shape)}")
        w = wave.to(device=self.device, dtype=torch.float32).reshape(-1, wave.shape[-1]).contiguous()
        B, n = int(w.shape[0]), int(w.shape[1])
        N = self.num_frames(n)
        if N < 1:
            raise ValueError(f"MelSpectrogram needs at least max({self.n_fft // 2 + 1}, {self.hop}) samples, got {n}")
        out = torch.empty(B, N, self.n_mels, device=self.device, dtype=torch.float32)
        cur = torch.cuda.current_stream(self.device)
        if cur != self._stream:
            self._stream.wait_stream(cur)
        _lib.check(self._lib.dsh_mel_compute(self._h, w.data_ptr(), B, n, out.data_ptr()), "dsh_mel_compute")
        if cur != self._stream:
            cur.wait_stream(self._stream)
            w.record_stream(self._stream)
            out.record_stream(self._stream)
        return out[0] if wave.dim() == 1 else out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dsh_mel_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- HuBERT encoder -------------------------------------------------------------------------------------------------------------------------
class HubertConfigC(C.Structure):
    _fields_ = [("hidden", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32), ("intermediate", C.c_int32),
                ("conv_dim", C.c_int32 * 7), ("conv_kernel", C.c_int32 * 7), ("conv_stride", C.c_int32 * 7),
                ("pos_kernel", C.c_int32), ("pos_groups", C.c_int32), ("ln_eps", C.c_float)]


HUBERT_LARGE = dict(hidden=1024, layers=24, heads=16, intermediate=4096, conv_dim=(512,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2),
                    conv_stride=(5, 2, 2, 2, 2, 2, 2), pos_kernel=128, pos_groups=16, ln_eps=1e-5)
HUBERT_CHUNK = 320000            # get_hubert_from_16k_speech_long: clips of 1000 frames (20 s) ...
HUBERT_CONTEXT = 80              # ... plus kernel - stride = 400 - 320 samples, so that consecutive clips neither overlap nor leave a gap
PACKED_KINDS = dict(conv=0, feat_proj=1, pos_conv=2, qkv=3, out_proj=4, ffn_in=5, ffn_out=6)


def hubert_config_c(config: dict) -> HubertConfigC:
    c = HubertConfigC()
    for k in ("hidden", "layers", "heads", "intermediate", "pos_kernel", "pos_groups"):
        setattr(c, k, int(config[k]))
    for k in ("conv_dim", "conv_kernel", "conv_stride"):
        if len(config[k]) != 7:
            raise ValueError(f"HubertEncoder: {k} must have 7 entries (the feature extractor has seven convolutions)")
        setattr(c, k, (C.c_int32 * 7)(*[int(v) for v in config[k]]))
    c.ln_eps = float(config.get("ln_eps", 1e-5))
    return c


class HubertEncoder:
    """transformers' ``HubertModel`` of the hubert-large family on the device (csrc/hubert.hip): ``HubertEncoder(HubertEncoder.LARGE)
    .load_state_dict(HubertModel.from_pretrained(..).state_dict())``; ``encode(x)`` is ``model(x).last_hidden_state`` for an already
    normalised ``x [B, n]``, ``encode_long(wave16k)`` the reference's chunked ``get_hubert_from_16k_speech_long``.  ``config`` is a dict
    with ``hidden, layers, heads, intermediate, conv_dim[7], conv_kernel[7], conv_stride[7], pos_kernel, pos_groups, ln_eps``."""

    LARGE = HUBERT_LARGE

    def __init__(self, config: dict = HUBERT_LARGE, device="cuda:0"):
        self.config = dict(config)
        self.hidden = int(config["hidden"])
        self._lib = _lib.lib()
        self.device = torch.device(device) if device is not None else None
        stream = 0
        if self.device is not None and torch.cuda.is_available():
            torch.cuda.set_device(self.device)
            self._stream = torch.cuda.current_stream(self.device)
            stream = self._stream.cuda_stream
        self._h = C.c_void_p()
        cfg = hubert_config_c(config)
        _lib.check(self._lib.dsh_hubert_create(C.byref(cfg), C.c_void_p(stream), C.byref(self._h)), "dsh_hubert_create")
        self.finalized = False

    def load_tensors(self, state_dict) -> "HubertEncoder":
        """Host side only (needs no device): every floating-point tensor by its key; a leading ``hubert.`` (``HubertForCTC``) is stripped."""
        for name, t in state_dict.items():
            if not torch.is_floating_point(t):
                continue
            if name.startswith("hubert."):
                name = name[len("hubert."):]
            a = t.detach().to("cpu", torch.float32).contiguous()
            shape = (C.c_int64 * max(a.dim(), 1))(*a.shape)
            _lib.check(self._lib.dsh_hubert_load_tensor(self._h, name.encode(), C.c_void_p(a.data_ptr()), shape, a.dim()),
                       f"dsh_hubert_load_tensor({name})")
        return self

    def load_state_dict(self, state_dict) -> "HubertEncoder":
        self.load_tensors(state_dict)
        _lib.check(self._lib.dsh_hubert_finalize(self._h), "dsh_hubert_finalize")
        self.finalized = True
        return self

    def packed(self, kind: str, layer: int = 0):
        """Test helper (host only, before the weights are finalized): ``(W [N, K], bias [N], fc [N])`` of one Linear / convolution as
        ``dsh_hubert_finalize`` would upload it; ``kind`` one of ``PACKED_KINDS``."""
        dims = (C.c_int32 * 2)()
        _lib.check(self._lib.dsh_hubert_debug_packed(self._h, PACKED_KINDS[kind], layer, dims, None, None, None), "dsh_hubert_debug_packed")
        W = np.empty((dims[0], dims[1]), dtype=np.float32)
        b = np.empty((dims[0],), dtype=np.float32)
        c = np.empty((dims[0],), dtype=np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.dsh_hubert_debug_packed(self._h, PACKED_KINDS[kind], layer, dims, p(W), p(b), p(c)), "dsh_hubert_debug_packed")
        return W, b, c

    def num_frames(self, n: int) -> int:
        return int(self._lib.dsh_hubert_num_frames(self._h, int(n)))

    def set_chunk_pass(self, rows: int) -> None:
        _lib.check(self._lib.dsh_hubert_set_chunk_pass(self._h, int(rows)), "dsh_hubert_set_chunk_pass")

    def encode(self, x: torch.Tensor) -> torch.Tensor:
        """``[B, n]`` (or ``[n]``) normalised samples -> ``[B, M, hidden]`` (``[M, hidden]``) fp32 on the device."""
        if not self.finalized:
            raise _lib.DshError("HubertEncoder.encode: load_state_dict first")
        if x.dim() not in (1, 2):
            raise ValueError(f"HubertEncoder.encode takes [n] or [B, n], got {tuple(x.shape)}")
        w = x.to(device=self.device, dtype=torch.float32).reshape(-1, x.shape[-1]).contiguous()
        B, n = int(w.shape[0]), int(w.shape[1])
        M = self.num_frames(n)
        if M < 1:
            raise ValueError(f"HubertEncoder.encode: {n} samples are shorter than the receptive field")
        out = torch.empty(B, M, self.hidden, device=self.device, dtype=torch.float32)
        cur = torch.cuda.current_stream(self.device)
        if cur != self._stream:
            self._stream.wait_stream(cur)
        _lib.check(self._lib.dsh_hubert_encode(self._h, w.data_ptr(), B, n, out.data_ptr()), "dsh_hubert_encode")
        if cur != self._stream:
            cur.wait_stream(self._stream)
            w.record_stream(self._stream)
            out.record_stream(self._stream)
        return out[0] if x.dim() == 1 else out

    def encode_long(self, wave16k: torch.Tensor) -> torch.Tensor:
        """``get_hubert_from_16k_speech_long`` of the reference: normalise the whole utterance, encode it in clips of 320 000 + 80 samples
        (all full clips as ONE batch) plus the remainder if it has 400 samples, concatenate, cut or zero-pad to ``(n - 80) // 320`` rows."""
        return chunked_encode(self.encode, normalize_wave(wave16k.reshape(-1)))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dsh_hubert_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def chunked_encode(encode, x: torch.Tensor) -> torch.Tensor:
    """The chunking rule of ``get_hubert_from_16k_speech_long`` for a normalised signal ``x [n]`` and ``encode([B, m]) -> [B, M, hidden]``."""
    n, c = int(x.shape[0]), HUBERT_CHUNK
    pieces = [x[i * c:i * c + c + HUBERT_CONTEXT] for i in range(n // c)]      # (a slice clamps: the last one may be shorter)
    whole = [p for p in pieces if p.shape[0] == c + HUBERT_CONTEXT]
    parts = list(encode(torch.stack(whole))) if whole else []
    parts += [encode(p[None])[0] for p in pieces if p.shape[0] != c + HUBERT_CONTEXT]
    if n - (n // c) * c >= 400:
        parts.append(encode(x[(n // c) * c:][None])[0])
    if not parts:
        raise ValueError(f"chunked_encode: {n} samples are shorter than the receptive field (400)")
    out = torch.cat(parts, 0)
    want = (n - HUBERT_CONTEXT) // 320
    if abs(int(out.shape[0]) - want) > 1:
        raise ValueError(f"chunked_encode: {int(out.shape[0])} encoder rows where {want} are expected")
    if out.shape[0] < want:
        out = torch.cat((out, out.new_zeros(want - out.shape[0], out.shape[1])), 0)
    return out[:want]


class AudioFrontEnd:
    """The two conditioning features of ``test_custom_aud`` from a 16 kHz signal, on the device:
    ``mel, hub = AudioFrontEnd(hubert).features(wave16k)`` gives ``mel [N, 128]`` (of the signal resampled to 18 kHz by 9 / 8, or of
    ``wave18k=`` if the caller has one) and ``hub [N, hidden]`` (the chunked HuBERT rows, 50 per second, interpolated linearly in time to
    the ``N = len18k // 1200`` mel frames as the reference's ``F.interpolate(.., align_corners=True)`` does)."""

    def __init__(self, hubert: HubertEncoder, device=None):
        self.hubert = hubert
        self.device = torch.device(device) if device is not None else hubert.device
        self.mel = MelSpectrogram(device=self.device)

    def features(self, wave16k: torch.Tensor, wave18k: torch.Tensor = None):
        w16 = wave16k.to(device=self.device, dtype=torch.float32).reshape(-1)
        w18 = resample_poly(w16, 9, 8) if wave18k is None else wave18k.to(device=self.device, dtype=torch.float32).reshape(-1)
        mel = self.mel(w18)
        N = int(mel.shape[0])
        hub = self.hubert.encode_long(w16).contiguous()
        out = torch.empty(N, hub.shape[1], device=self.device, dtype=torch.float32)
        _lib.check(_lib.lib().dsh_interp_time(_stream(self.device), hub.data_ptr(), 1, int(hub.shape[0]), int(hub.shape[1]), out.data_ptr(), N),
                   "dsh_interp_time")
        return mel, out
