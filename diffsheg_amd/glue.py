"""Rows either side of the sampling path (SURVEY.md §8f "next"), to the same drop-in standard:

* :func:`load_checkpoint` — the reference's ``.tar`` (``torch.save`` dict, weights under ``['encoder']``,
  DDP ``module.`` prefix tolerated, ``strict=False``; /root/reference/trainers/ddpm_show_trainer.py:259-292);
* :func:`interpolate_features` — HuBERT hidden states resampled to the pose frame rate with
  ``F.interpolate(mode='linear', align_corners=True)`` (datasets/show.py:98, ddpm_show_trainer.py:1082), HIP kernel;
* :func:`inv_standardize` / :func:`split_motion` — de-normalisation and gesture|expression split of the sampled
  window chain (datasets/show.py:157-162, ddpm_show_trainer.py:906-921), HIP kernel, output stays on the device;
* :func:`axis_angle_to_euler` / :func:`euler_to_axis_angle` with :class:`PoseStats` — the BEAT results tail: the sampled gesture
  channels (standardised axis-angle, ``--axis_angle``) to the standardised Euler 'XYZ' degrees the reference saves, scores and writes
  to BVH (ddpm_beat_trainer.py:1044-1060, datasets/rotation_converter.py), and the dataset's opposite direction
  (datasets/beat.py:376-401) for frames a caller holds as Euler / BVH poses; HIP kernels, output stays on the device.

* :func:`edit_region` — the keep mask of an edit (``DDPMTrainer.sample_variations(keep=)``) from frame and column ranges, HIP kernel.

HuBERT itself (``facebook/hubert-large-ls960-ft``), mel extraction and the BVH / face-JSON file writers (they need the dataset's
template files) stay out of scope.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib
from .weights import strip_ddp_prefix


def load_checkpoint(path: str) -> Tuple[Dict[str, torch.Tensor], Dict[str, object]]:
    """Return (UniDiffuser state dict, metadata) from a reference checkpoint file."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    if "encoder" not in ckpt:
        raise KeyError("checkpoint has no 'encoder' entry (expected the dict written by DDPMTrainer_*.save)")
    meta = {k: ckpt.get(k) for k in ("ep", "total_it", "best_fgd", "best_mse", "best_pck") if k in ckpt}
    return strip_ddp_prefix(ckpt["encoder"]), meta


def _stream_ptr(device: torch.device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def interpolate_features(feat: torch.Tensor, frames_out: int) -> torch.Tensor:
    """[B, T_in, C] (or [T_in, C]) fp32 on a GPU -> [B, frames_out, C], linear with align_corners=True."""
    if not feat.is_cuda:
        raise _lib.DshError("interpolate_features runs on the GPU (no CPU fallback)")
    squeeze = feat.dim() == 2
    x = (feat.unsqueeze(0) if squeeze else feat).to(torch.float32).contiguous()
    B, Tin, Cc = x.shape
    y = torch.empty(B, frames_out, Cc, device=x.device)
    _lib.check(_lib.lib().dsh_interp_time(_stream_ptr(x.device), x.data_ptr(), B, Tin, Cc, y.data_ptr(), frames_out),
               "dsh_interp_time")
    return y.squeeze(0) if squeeze else y


def inv_standardize(motion: torch.Tensor, mean: torch.Tensor, std: torch.Tensor) -> torch.Tensor:
    """``motion * std + mean`` over the channel (last) axis, on the device."""
    if not motion.is_cuda:
        raise _lib.DshError("inv_standardize runs on the GPU (no CPU fallback)")
    x = motion.to(torch.float32).contiguous()
    Cc = x.shape[-1]
    m = mean.to(device=x.device, dtype=torch.float32).reshape(-1).contiguous()
    s = std.to(device=x.device, dtype=torch.float32).reshape(-1).contiguous()
    if m.numel() != Cc or s.numel() != Cc:
        raise ValueError(f"mean/std must have {Cc} entries")
    y = torch.empty_like(x)
    _lib.check(_lib.lib().dsh_inv_standardize(_stream_ptr(x.device), x.data_ptr(), x.numel(), Cc, m.data_ptr(), s.data_ptr(),
                                              y.data_ptr()), "dsh_inv_standardize")
    return y


def split_motion(motion: torch.Tensor, split_pos: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """gesture | expression split of the joint motion tensor (ddpm_show_trainer.py:920-921)."""
    return motion[..., :split_pos], motion[..., split_pos:]


class PoseStats:
    """The four BEAT pose statistics of the Euler tail: mean / std of the axis-angle channels (the reference's
    ``mean_pose_axis_angle`` / ``std_pose_axis_angle``) and of the Euler channels in degrees (``mean_pose`` / ``std_pose``), each
    ``[3 J]``.  Inputs are host or device tensors, numpy arrays or sequences of any float dtype; they are kept as flat fp32 vectors and
    moved to ``device`` (now when given, otherwise to the device of the first tensor converted with them)."""

    FIELDS = ("mean_axis_angle", "std_axis_angle", "mean_euler", "std_euler")

    def __init__(self, mean_axis_angle, std_axis_angle, mean_euler, std_euler, device=None):
        vecs = [torch.as_tensor(v).detach().to(torch.float32).reshape(-1).contiguous()
                for v in (mean_axis_angle, std_axis_angle, mean_euler, std_euler)]
        n = vecs[0].numel()
        if n == 0 or n % 3 != 0 or any(v.numel() != n for v in vecs):
            raise ValueError(f"PoseStats needs four vectors of one length 3 J, got {[v.numel() for v in vecs]}")
        self.channels = n
        self.mean_axis_angle, self.std_axis_angle, self.mean_euler, self.std_euler = vecs
        if device is not None:
            self.to(device)

    def to(self, device) -> "PoseStats":
        """Move the four vectors to ``device`` (in place; nothing happens when they are there already); returns ``self``."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.mean_axis_angle.device != device:
            for name in PoseStats.FIELDS:
                setattr(self, name, getattr(self, name).to(device))
        return self


def _rotation_call(which: str, x: torch.Tensor, stats: PoseStats, split_pos: Optional[int], lengths, raw: bool) -> torch.Tensor:
    """Shared front of the two conversions: argument checks (ValueError), no CPU path (DshError), one launch reading ``x`` in place."""
    if not isinstance(stats, PoseStats):
        raise ValueError(f"{which} needs a PoseStats, got {type(stats).__name__}")
    if x.dim() < 1:
        raise ValueError(f"{which} takes [..., channels] tensors")
    Cc = int(x.shape[-1])
    n = Cc if split_pos is None else int(split_pos)
    if n < 3 or n > Cc or n % 3 != 0:
        raise ValueError(f"{which}: {n} rotation channels of {Cc} (need a multiple of 3, at least one joint, at most the tensor's width)")
    if stats.channels != n:
        raise ValueError(f"{which}: the statistics have {stats.channels} entries, the rotation channels are {n}")
    lens = None
    if lengths is not None:
        if x.dim() < 2:
            raise ValueError(f"{which}: lengths need a [..., T, channels] tensor")
        T = int(x.shape[-2])
        lens = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        clips = x.numel() // (T * Cc) if T * Cc else 0
        if len(lens) != clips or any(v < 1 or v > T for v in lens):
            raise ValueError(f"{which}: lengths needs one frame count in 1 .. {T} per clip ({clips}), got {lens}")
    if not x.is_cuda:
        raise _lib.DshError(f"{which} runs on the GPU (no CPU fallback)")
    src = x.to(torch.float32).contiguous()
    out = torch.empty_like(src)
    if n < Cc:
        out[..., n:] = src[..., n:]
    m_aa, s_aa, m_e, s_e = (getattr(stats.to(src.device), name).data_ptr() for name in PoseStats.FIELDS)
    rows = src.numel() // Cc
    ld, T = Cc, (int(src.shape[-2]) if lens is not None else 0)
    lens_dev = torch.tensor(lens, dtype=torch.int32).to(src.device) if lens is not None else None
    lp = lens_dev.data_ptr() if lens_dev is not None else None
    with torch.cuda.device(src.device):
        if which == "axis_angle_to_euler":
            y_std, y_deg = (None, out.data_ptr()) if raw else (out.data_ptr(), None)
            rc = _lib.lib().dsh_axis_angle_to_euler(_stream_ptr(src.device), src.data_ptr(), ld, rows, n // 3, m_aa, s_aa, m_e, s_e,
                                                    y_std, ld, y_deg, ld, lp, T)
        else:
            rc = _lib.lib().dsh_euler_to_axis_angle(_stream_ptr(src.device), src.data_ptr(), ld, rows, n // 3, m_e, s_e, m_aa, s_aa,
                                                    out.data_ptr(), ld, lp, T)
    _lib.check(rc, "dsh_" + which)
    return out


def axis_angle_to_euler(motion: torch.Tensor, stats: PoseStats, *, split_pos: Optional[int] = None, lengths: Optional[Sequence[int]] = None,
                        degrees: bool = False) -> torch.Tensor:
    """The reference's BEAT results tail (ddpm_beat_trainer.py:1044-1060) on the device: standardised axis-angle channels
    ``[..., 3 J]`` -> de-normalise with the axis-angle statistics -> ``axis_angle_to_euler_angles`` (convention 'XYZ') -> degrees ->
    re-normalise with the Euler statistics.  ``degrees=True`` returns the plain degrees instead (what goes into a BVH).

    ``split_pos``: ``motion`` is the joint ``[..., C]`` tensor (gesture | expression); its first ``split_pos`` channels are converted,
    read in place from the wide rows, and the channels behind are returned unchanged, in a new tensor.  ``lengths`` (one frame count in
    ``1 .. T`` per clip of a ``[..., T, C]`` tensor): frames behind a clip's length are exact zeros in the converted channels, whatever
    the input holds there — the ragged sampler's convention for padded frames (channels behind ``split_pos`` are copied as they are:
    the sampler's pad is 0 already).  One deviation from the reference: a joint at gimbal lock gives a
    middle angle of +-90 degrees where the reference's fp32 run gives NaN once R02 rounds past 1."""
    return _rotation_call("axis_angle_to_euler", motion, stats, split_pos, lengths, bool(degrees))


def euler_to_axis_angle(pose: torch.Tensor, stats: PoseStats, *, split_pos: Optional[int] = None,
                        lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
    """The dataset's direction (datasets/beat.py:376-401): standardised Euler 'XYZ' degrees ``[..., 3 J]`` -> de-normalise -> radians ->
    ``euler_angles_to_axis_angle(..., 'XYZ')`` -> normalise with the axis-angle statistics: what ``motions``, ``head`` and ``tail`` of
    the samplers expect from frames held as Euler / BVH poses.  ``split_pos`` / ``lengths`` as for :func:`axis_angle_to_euler`."""
    return _rotation_call("euler_to_axis_angle", pose, stats, split_pos, lengths, False)


def _ranges(v, what: str, hi: int):
    out = [(int(a), int(b)) for a, b in v]
    for a, b in out:
        if not 0 <= a <= b <= hi:
            raise ValueError(f"edit_region: {what} range ({a}, {b}) outside 0 <= lo <= hi <= {hi}")
    return out


def edit_region(B: int, T: int, C_: int, frames=None, columns=None, device="cuda") -> torch.Tensor:
    """The keep mask of an edit, built on the device in one launch: a bool tensor ``[B, T, C]``, False (re-sample) where the frame lies
    in one of the ``frames`` ranges OR the column in one of the ``columns`` ranges, True (leave as it is) elsewhere — "re-roll seconds
    3-5 and the hands, keep the rest".  ``frames``: a list (of tuples or lists) of half-open ``(a, b)`` ranges, ALL of them shared by every row, or
    a ``[B, 2]`` tensor with one range per row (only a tensor is read per row); ``columns``: a list of half-open ``(lo, hi)`` ranges.  Ranges are validated on the host
    (``ValueError``); an empty range edits nothing."""
    B, T, C_ = int(B), int(T), int(C_)
    if B < 1 or T < 1 or C_ < 1:
        raise ValueError(f"edit_region needs a positive shape, got {(B, T, C_)}")
    per_row = None
    if frames is not None:
        if isinstance(frames, torch.Tensor):
            if tuple(frames.shape) != (B, 2):
                raise ValueError(f"edit_region: a frames tensor holds one range per row, [{B}, 2], got {tuple(frames.shape)}")
            per_row = [[r] for r in _ranges(frames.detach().to("cpu").tolist(), "frame", T)]
        else:
            shared = _ranges(frames, "frame", T)
            per_row = [shared] * B
    nf = len(per_row[0]) if per_row else 0
    cols = _ranges(columns, "column", C_) if columns is not None else []
    nc = len(cols)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.DshError("edit_region runs on the GPU (no CPU fallback)")
    flat_f = [v for row in (per_row or []) for r in row for v in r]
    flat_c = [v for r in cols for v in r]
    host = torch.tensor(flat_f + flat_c + [0], dtype=torch.int32)
    devt = host.to(dev)
    keep = torch.empty(B, T, C_, dtype=torch.uint8, device=dev)
    fh = (C.c_int32 * max(len(flat_f), 1))(*flat_f)
    ch = (C.c_int32 * max(len(flat_c), 1))(*flat_c)
    with torch.cuda.device(dev):
        rc = _lib.lib().dsh_op_region_mask(_stream_ptr(keep.device), fh, devt.data_ptr() if nf else None, nf, ch,
                                           devt.data_ptr() + 4 * len(flat_f) if nc else None, nc, B, T, C_, keep.data_ptr())
    _lib.check(rc, "dsh_op_region_mask")
    return keep.view(torch.bool)
