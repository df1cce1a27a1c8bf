"""Audio front on the device (csrc/audio_front.hip): what the reference's ``test_custom_aud`` (trainers/ddpm_show_trainer.py:944-1100,
ddpm_beat_trainer.py:1123-1340) computes from a speech signal in front of the sampler.

    mel   = MelSpectrogram()(wave18k)            # [N, 128], N = len // 1200: librosa.feature.melspectrogram(..)[..., :-1]
    w18k  = resample_poly(wave16k, 9, 8)         # scipy.signal.resample_poly semantics

Utterances of different durations go through in one call: ``lengths=`` (one sample count per row of a zero-padded ``[B, n]``) on
``MelSpectrogram.__call__``, ``resample_poly`` and ``HubertEncoder.encode``; ``AudioFrontEnd.features_batch(list of signals)`` on top of them.
Row ``b`` of every result is bit for bit the single-signal call on its own samples, and 0 behind its own frames.

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


def _row_lengths(lengths, B: int, n: int, what: str) -> list:
    """one sample count per row of a ``[B, n]`` batch, as a list of ints"""
    lens = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
    if len(lens) != B:
        raise ValueError(f"{what}: {len(lens)} lengths for {B} rows")
    if any(v > n for v in lens):
        raise ValueError(f"{what}: a length of {max(lens)} samples in rows of {n}")
    return lens


def _lens_dev(lens, device) -> torch.Tensor:
    return torch.tensor(lens, dtype=torch.int32).to(device)


def pad_waves(waves, device) -> tuple:
    """a list of signals ``[n_b]`` -> (``[B, max n_b]`` fp32 on ``device``, zero-padded; the list of ``n_b``)"""
    ws = [w.to(device=device, dtype=torch.float32).reshape(-1) for w in waves]
    if not ws:
        raise ValueError("an empty list of signals")
    return torch.nn.utils.rnn.pad_sequence(ws, batch_first=True), [int(w.shape[0]) for w in ws]


def resample_poly(x: torch.Tensor, up: int, down: int, taps=None, lengths=None) -> torch.Tensor:
    """``scipy.signal.resample_poly(x, up, down)`` along the last axis of ``x [n]`` or ``[B, n]`` (device fp32) on the device.  ``taps``
    (odd length, gain included; default :func:`resample_taps`) are rounded to fp32.  The reference resamples with resampy's
    ``kaiser_best`` filter instead: same band, other taps.  ``lengths`` (one sample count per row of a padded ``[B, n]``): row ``b`` is the
    call on ``x[b, :lengths[b]]`` alone, 0 behind its ``ceil(lengths[b] up / down)`` samples; the padding is never read."""
    if not x.is_cuda:
        raise _lib.DshError("resample_poly runs on the GPU: there is no CPU fallback")
    g = math.gcd(int(up), int(down))
    up, down = int(up) // g, int(down) // g
    x2 = x.to(torch.float32).reshape(-1, x.shape[-1]).contiguous()
    lens = None if lengths is None else _row_lengths(lengths, int(x2.shape[0]), int(x2.shape[1]), "resample_poly")
    if lens is not None and min(lens) < 1:
        raise ValueError("resample_poly: every row needs at least one sample")
    if up == down:
        if lens is not None:
            x2 = torch.where(torch.arange(x2.shape[1], device=x2.device)[None] < _lens_dev(lens, x2.device)[:, None], x2, torch.zeros_like(x2))
        return x2.clone().reshape(x.shape)
    h = resample_taps(up, down) if taps is None else np.asarray(taps, dtype=np.float64)
    if h.ndim != 1 or h.shape[0] % 2 != 1:
        raise ValueError("resample_poly takes an odd number of taps")
    B, n = int(x2.shape[0]), int(x2.shape[1])
    L = _lib.lib()
    n_out = int(L.dsh_resample_poly_len(n, up, down))
    taps_dev = torch.from_numpy(h.astype(np.float32)).to(x2.device)
    y = torch.empty(B, n_out, device=x2.device, dtype=torch.float32)
    if lens is None:
        _lib.check(L.dsh_op_resample_poly(_stream(x2.device), x2.data_ptr(), B, n, up, down, taps_dev.data_ptr(), int(h.shape[0]), y.data_ptr()),
                   "dsh_op_resample_poly")
    else:
        ld = _lens_dev(lens, x2.device)
        _lib.check(L.dsh_op_resample_poly_ragged(_stream(x2.device), x2.data_ptr(), B, n, ld.data_ptr(), up, down, taps_dev.data_ptr(),
                                                 int(h.shape[0]), y.data_ptr()), "dsh_op_resample_poly_ragged")
    return y.reshape(tuple(x.shape[:-1]) + (n_out,))


class MelSpectrogram:
    """``librosa.feature.melspectrogram(y, sr=18000, hop_length=1200, n_mels=128)[..., :-1]`` transposed to frames-first, as the reference
    feeds it to the model: ``mel = MelSpectrogram()(wave)`` for ``wave [len]`` or ``[B, len]`` gives ``[len // 1200, 128]`` or
    ``[B, len // 1200, 128]`` fp32 on the device (power spectrogram, no logarithm).  Needs ``len >= 1200``.  ``mel(wave, lengths=)`` takes a
    padded ``[B, len]`` with one sample count per row: row ``b`` is ``mel(wave[b, :lengths[b]])`` bit for bit in its first
    ``lengths[b] // 1200`` frames and 0 behind; the padding is never read."""

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

    def __call__(self, wave: torch.Tensor, lengths=None) -> torch.Tensor:
        if self.device is None:
            raise _lib.DshError("MelSpectrogram was created without a device: there is no CPU fallback")
        if wave.dim() not in (1, 2):
            raise ValueError(f"MelSpectrogram takes [len] or [B, len], got {tuple(wave.shape)}")
        w = wave.to(device=self.device, dtype=torch.float32).reshape(-1, wave.shape[-1]).contiguous()
        B, n = int(w.shape[0]), int(w.shape[1])
        N = self.num_frames(n)
        if N < 1:
            raise ValueError(f"MelSpectrogram needs at least max({self.n_fft // 2 + 1}, {self.hop}) samples, got {n}")
        ld = None
        if lengths is not None:
            lens = _row_lengths(lengths, B, n, "MelSpectrogram")
            if min(self.num_frames(v) for v in lens) < 1:
                raise ValueError(f"MelSpectrogram needs at least max({self.n_fft // 2 + 1}, {self.hop}) samples per row, got {min(lens)}")
            ld = _lens_dev(lens, self.device)
        out = torch.empty(B, N, self.n_mels, device=self.device, dtype=torch.float32)
        cur = torch.cuda.current_stream(self.device)
        if cur != self._stream:
            self._stream.wait_stream(cur)
        if ld is None:
            _lib.check(self._lib.dsh_mel_compute(self._h, w.data_ptr(), B, n, out.data_ptr()), "dsh_mel_compute")
        else:
            _lib.check(self._lib.dsh_mel_compute_ragged(self._h, w.data_ptr(), B, n, ld.data_ptr(), out.data_ptr()), "dsh_mel_compute_ragged")
        if cur != self._stream:
            cur.wait_stream(self._stream)
            w.record_stream(self._stream)
            out.record_stream(self._stream)
            if ld is not None:
                ld.record_stream(self._stream)
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

    PRECISIONS = {"fp32": 0, "bf16": 1}

    def __init__(self, config: dict = HUBERT_LARGE, device="cuda:0", precision: str = "fp32"):
        """``precision="bf16"``: the transformer layers on the bf16 matrix pipe (``dsh_hubert_set_precision``); the convolution stack, the
        projection, the positional convolution and the last LayerNorm stay fp32, and so do the outputs.  Every method follows it."""
        if precision not in self.PRECISIONS:
            raise ValueError(f"HubertEncoder: precision must be one of {sorted(self.PRECISIONS)}, got {precision!r}")
        self.precision = precision
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
        if precision != "fp32":
            _lib.check(self._lib.dsh_hubert_set_precision(self._h, self.PRECISIONS[precision]), "dsh_hubert_set_precision")
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

    def debug_tap(self, h_posconv: torch.Tensor = None) -> None:
        """Test helper: every following ``encode`` copies the residual stream ``[B M, hidden]`` as the positional convolution leaves it into
        this fp32 device tensor (the caller keeps it alive and large enough); ``None`` switches the tap off."""
        _lib.check(self._lib.dsh_hubert_debug_tap(self._h, None if h_posconv is None else h_posconv.data_ptr()), "dsh_hubert_debug_tap")

    def set_chunk_pass(self, rows: int) -> None:
        _lib.check(self._lib.dsh_hubert_set_chunk_pass(self._h, int(rows)), "dsh_hubert_set_chunk_pass")

    def encode(self, x: torch.Tensor, lengths=None) -> torch.Tensor:
        """``[B, n]`` (or ``[n]``) normalised samples -> ``[B, M, hidden]`` (``[M, hidden]``) fp32 on the device.  ``lengths`` (one sample
        count per row of a padded ``[B, n]``, each at least the receptive field): frames ``t < num_frames(lengths[b])`` of row ``b`` are
        ``encode(x[b, :lengths[b]])`` bit for bit, the frames behind are 0, whatever the padding holds."""
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
        if lengths is None:
            _lib.check(self._lib.dsh_hubert_encode(self._h, w.data_ptr(), B, n, out.data_ptr()), "dsh_hubert_encode")
        else:
            lens = _row_lengths(lengths, B, n, "HubertEncoder.encode")
            if min(self.num_frames(v) for v in lens) < 1:
                raise ValueError(f"HubertEncoder.encode: a row of {min(lens)} samples is shorter than the receptive field")
            _lib.check(self._lib.dsh_hubert_encode_ragged(self._h, w.data_ptr(), B, n, (C.c_int64 * B)(*lens), out.data_ptr()),
                       "dsh_hubert_encode_ragged")
        if cur != self._stream:
            cur.wait_stream(self._stream)
            w.record_stream(self._stream)
            out.record_stream(self._stream)
        return out[0] if x.dim() == 1 else out

    def encode_long(self, wave16k: torch.Tensor) -> torch.Tensor:
        """``get_hubert_from_16k_speech_long`` of the reference: normalise the whole utterance, encode it in clips of 320 000 + 80 samples
        (all full clips as ONE batch) plus the remainder if it has 400 samples, concatenate, cut or zero-pad to ``(n - 80) // 320`` rows."""
        return chunked_encode(self.encode, normalize_wave(wave16k.reshape(-1)))

    def encode_long_batch(self, waves, min_fill: float = None) -> list:
        """:meth:`encode_long` of every signal of a list, bit for bit, in two encoder passes instead of one or two per signal: every
        utterance is normalised on its own, all full clips of all utterances go through one ``encode``, all remainders (padded to the
        longest) through one ``encode(.., lengths=)``.  Returns the list of ``[(n_b - 80) // 320, hidden]``.  The Linears of the ragged
        pass run on the padded rows, so remainders of very different lengths pay for the padding; ``min_fill`` (0 .. 1) splits them into
        as many ragged passes as :func:`length_groups` needs for every remainder to fill that share of its pass.  The bits do not depend
        on it."""
        xs = [normalize_wave(w.to(self.device).reshape(-1)) for w in waves]
        full, rest = plan_chunks([int(x.shape[0]) for x in xs])
        c = HUBERT_CHUNK
        parts = [[] for _ in xs]
        if full:
            rows = self.encode(torch.stack([xs[u][i * c:i * c + c + HUBERT_CONTEXT] for u, i in full]))
            for k, (u, _) in enumerate(full):                 # (plan_chunks lists an utterance's clips in order)
                parts[u].append(rows[k])
        for group in length_groups([cnt for _, _, cnt in rest], min_fill):
            batch, counts = pad_waves([xs[rest[k][0]][rest[k][1]:rest[k][1] + rest[k][2]] for k in group], self.device)
            rows = self.encode(batch, lengths=counts)
            for j, k in enumerate(group):
                parts[rest[k][0]].append(rows[j, :self.num_frames(rest[k][2])])
        return [_fit_rows(torch.cat(p, 0), int(x.shape[0])) for p, x in zip(parts, xs)]

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dsh_hubert_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def plan_chunks(sample_counts) -> tuple:
    """The chunking rule of ``get_hubert_from_16k_speech_long`` (:func:`chunked_encode`) for many utterances at once, on the host:
    ``(full, rest)`` with ``full`` the ``(utterance, chunk index)`` of every full clip ``x[i c : i c + c + 80]`` (``c`` = 320 000) and
    ``rest`` the ``(utterance, offset, count)`` of every shorter piece of at least 400 samples that the rule encodes on its own: the
    remainder ``x[(n // c) c :]``, or a last clip that fewer than 80 samples follow.  Each utterance's entries are in encoding order, all
    its full clips in front of its remainder.  An utterance shorter than 400 samples is refused."""
    c, full, rest = HUBERT_CHUNK, [], []
    for u, n in enumerate(int(v) for v in sample_counts):
        if n < 400:
            raise ValueError(f"plan_chunks: utterance {u} has {n} samples, fewer than the receptive field (400)")
        for i in range(n // c):
            if i * c + c + HUBERT_CONTEXT <= n:
                full.append((u, i))
            else:
                rest.append((u, i * c, n - i * c))
        if n - (n // c) * c >= 400:
            rest.append((u, (n // c) * c, n - (n // c) * c))
    return full, rest


def length_groups(counts, min_fill: float = None) -> list:
    """Index groups of ``counts`` for padded passes: one group of everything when ``min_fill`` is None; otherwise the counts in descending
    order, a new group starting at the first count below ``min_fill`` times the group's longest.  Each group keeps ascending index order."""
    if not counts:
        return []
    if min_fill is None:
        return [list(range(len(counts)))]
    if not 0.0 <= float(min_fill) <= 1.0:
        raise ValueError(f"min_fill must lie in [0, 1], got {min_fill}")
    groups = []
    for k in sorted(range(len(counts)), key=lambda k: -counts[k]):
        if groups and counts[k] >= float(min_fill) * counts[groups[-1][0]]:
            groups[-1].append(k)
        else:
            groups.append([k])
    return [sorted(g) for g in groups]


def _fit_rows(out: torch.Tensor, n: int) -> torch.Tensor:
    """cut or zero-pad the concatenated encoder rows of an ``n``-sample utterance to ``(n - 80) // 320``"""
    want = (n - HUBERT_CONTEXT) // 320
    if abs(int(out.shape[0]) - want) > 1:
        raise ValueError(f"chunked_encode: {int(out.shape[0])} encoder rows where {want} are expected")
    if out.shape[0] < want:
        out = torch.cat((out, out.new_zeros(want - out.shape[0], out.shape[1])), 0)
    return out[:want]


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
    return _fit_rows(torch.cat(parts, 0), n)


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

    def features_batch(self, waves, waves18k=None, min_fill: float = None):
        """:meth:`features` of a list of 16 kHz signals of different durations in one pass over the front end: ``(mel [B, N_max, 128],
        hub [B, N_max, hidden], lengths)`` with ``lengths[b] = len18k_b // 1200``.  Row ``b`` restricted to its ``lengths[b]`` frames is
        bit for bit ``features(waves[b])``; the frames behind are 0 (what ``pad_sequence`` of the single results gives), ready for
        ``sample_arbitrary_len(.., lengths=lengths)``.  One ragged resampling, one ragged mel pass, the two encoder passes of
        :meth:`HubertEncoder.encode_long_batch` (more with its ``min_fill``) and one ragged interpolation, however many signals there
        are."""
        waves = [w.to(device=self.device, dtype=torch.float32).reshape(-1) for w in waves]
        w16, n16 = pad_waves(waves, self.device)
        if waves18k is None:
            w18 = resample_poly(w16, 9, 8, lengths=n16)
            n18 = [-(-n * 9 // 8) for n in n16]
        else:
            if len(waves18k) != len(n16):
                raise ValueError(f"features_batch: {len(waves18k)} 18 kHz signals for {len(n16)} signals")
            w18, n18 = pad_waves(waves18k, self.device)
        mel = self.mel(w18, lengths=n18)
        lengths = [n // self.mel.hop for n in n18]
        rows = self.hubert.encode_long_batch(waves, min_fill=min_fill)
        hub = torch.nn.utils.rnn.pad_sequence(rows, batch_first=True).contiguous()
        B, N = int(mel.shape[0]), int(mel.shape[1])
        out = torch.empty(B, N, hub.shape[2], device=self.device, dtype=torch.float32)
        lin, lout = _lens_dev([int(r.shape[0]) for r in rows], self.device), _lens_dev(lengths, self.device)
        _lib.check(_lib.lib().dsh_interp_time_ragged(_stream(self.device), hub.data_ptr(), B, int(hub.shape[1]), int(hub.shape[2]), out.data_ptr(), N,
                                                     lin.data_ptr(), lout.data_ptr()), "dsh_interp_time_ragged")
        return mel, out, lengths
