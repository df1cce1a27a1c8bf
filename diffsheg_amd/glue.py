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
* :func:`joint_positions` with :class:`Skeleton`, and :func:`position_metrics` — world-space joint positions of the gesture channels by
  forward kinematics on a caller-given skeleton, differentiable with respect to the motion (two HIP kernels), and MPJPE / PCK on them.

* :class:`CFGSchedule` — the classifier-free guidance weight per model timestep and per encoder, and the std rescale of the guided
  prediction (``UniDiffuser.set_guidance_schedule``, the loops' ``cfg_schedule=``); host-side tables.

* :func:`edit_region` — the keep mask of an edit (``DDPMTrainer.sample_variations(keep=)``) from frame and column ranges, HIP kernel.

HuBERT itself (``facebook/hubert-large-ls960-ft``), mel extraction and the BVH / face-JSON file writers (they need the dataset's
template files) stay out of scope.
"""
from __future__ import annotations

import copy
import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
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


# ---- forward kinematics: joint positions of the gesture channels and their gradient --------------------------------------
def _euler_deg_to_matrix(deg: np.ndarray) -> np.ndarray:
    """[..., 3] Euler degrees -> [..., 3, 3] = Rx(X) Ry(Y) Rz(Z), float64: the composition :func:`euler_to_axis_angle` uses."""
    a, b, c = np.moveaxis(np.radians(np.asarray(deg, dtype=np.float64)), -1, 0)
    sa, ca, sb, cb, sc, cc = np.sin(a), np.cos(a), np.sin(b), np.cos(b), np.sin(c), np.cos(c)
    m = [cb * cc, -cb * sc, sb,
         sa * sb * cc + ca * sc, ca * cc - sa * sb * sc, -sa * cb,
         sa * sc - ca * sb * cc, ca * sb * sc + sa * cc, ca * cb]
    return np.stack(m, -1).reshape(a.shape + (3, 3))


class Skeleton:
    """A rotation-only skeleton for :func:`joint_positions`, as arrays on the host (the dataset's template file is an input, not a
    committed asset):

    * ``parents`` int ``[J]``: ``parents[0] == -1``, ``parents[j] < j`` otherwise (topological order);
    * ``offsets`` ``[J, 3]``: a BVH's ``OFFSET`` lines; end sites are ordinary joints without channels;
    * ``channel_joint`` int ``[Jc]``: distinct joint indices, channel triple ``i`` of the motion drives joint ``channel_joint[i]``;
    * ``rest`` (optional) ``[J, 3]`` Euler degrees of the joints no channel drives (the template frame), folded here in float64 into
      ``rest_rot [J, 3, 3]`` by ``Rx Ry Rz``; identity by default.  The entries of driven joints are not used.

    ``ValueError``: a bad parent order, duplicate or out-of-range ``channel_joint``, non-finite offsets or rest angles, ``J < 1``,
    ``Jc < 1`` or ``J > 256``.  ``joint_channel`` is the inverse map (``-1`` where undriven), ``bone_length`` the sum of ``|offsets[j]|``
    over all joints (the root's offset, its position, included).  :meth:`to` uploads the five arrays once per device."""

    MAX_JOINTS = 256

    def __init__(self, parents, offsets, channel_joint, rest=None, names=None):
        par = np.asarray(parents)
        off = np.asarray(offsets, dtype=np.float64)
        cj = np.asarray(channel_joint)
        if par.ndim != 1 or par.size < 1 or par.size > Skeleton.MAX_JOINTS:
            raise ValueError(f"Skeleton: parents must be [J] with 1 <= J <= {Skeleton.MAX_JOINTS}, got shape {par.shape}")
        if par.dtype.kind not in "iu" or cj.dtype.kind not in "iu":
            raise ValueError("Skeleton: parents and channel_joint must be non-empty integer arrays")
        par, cj = par.astype(np.int64), cj.astype(np.int64)
        J = int(par.size)
        if par[0] != -1 or any(par[j] < 0 or par[j] >= j for j in range(1, J)):
            raise ValueError("Skeleton: parents[0] must be -1 and 0 <= parents[j] < j otherwise (topological order)")
        if off.shape != (J, 3) or not np.isfinite(off).all():
            raise ValueError(f"Skeleton: offsets must be finite [J, 3] = [{J}, 3], got shape {off.shape}")
        if cj.ndim != 1 or cj.size < 1:
            raise ValueError("Skeleton: channel_joint must be [Jc] with Jc >= 1")
        if cj.min() < 0 or cj.max() >= J or len(set(cj.tolist())) != cj.size:
            raise ValueError(f"Skeleton: channel_joint must hold distinct joint indices in 0 .. {J - 1}")
        rest_rot = np.broadcast_to(np.eye(3), (J, 3, 3)).copy()
        if rest is not None:
            r = np.asarray(rest, dtype=np.float64)
            if r.shape != (J, 3) or not np.isfinite(r).all():
                raise ValueError(f"Skeleton: rest must be finite [J, 3] = [{J}, 3] Euler degrees, got shape {r.shape}")
            rest_rot = _euler_deg_to_matrix(r)
        if names is not None and len(names) != J:
            raise ValueError(f"Skeleton: {len(names)} names for {J} joints")
        self.joints, self.channels = J, int(cj.size)
        self.parents, self.offsets, self.channel_joint, self.rest_rot = par.astype(np.int32), off, cj.astype(np.int32), rest_rot
        self.joint_channel = np.full(J, -1, dtype=np.int32)
        self.joint_channel[cj] = np.arange(cj.size, dtype=np.int32)
        self.names = list(names) if names is not None else None
        self.bone_length = float(np.sqrt((off ** 2).sum(-1)).sum())
        self._dev: Dict[torch.device, Dict[str, torch.Tensor]] = {}

    def to(self, device) -> Dict[str, torch.Tensor]:
        """The device buffers of the two C calls (int32 / fp32), uploaded on first use and kept."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._dev:
            self._dev[device] = {
                "parents": torch.from_numpy(self.parents).to(device),
                "offsets": torch.from_numpy(self.offsets.astype(np.float32)).contiguous().to(device),
                "channel_joint": torch.from_numpy(self.channel_joint).to(device),
                "rest_rot": torch.from_numpy(self.rest_rot.astype(np.float32)).contiguous().to(device),
                "joint_channel": torch.from_numpy(self.joint_channel).to(device)}
        return self._dev[device]

    @classmethod
    def from_bvh_header(cls, text: str, joints=None, rest=None) -> "Skeleton":
        """Parse the ``HIERARCHY`` block of a BVH file (everything up to ``MOTION``, if present) into a skeleton; a reader, not a
        writer.  ``ROOT`` / ``JOINT`` blocks and ``End Site`` blocks become joints in file order (an end site is named
        ``"<parent>_end"``).  ``joints``: the driven joints in channel order, as names or indices; by default every joint whose
        ``CHANNELS`` line names a rotation.  ``rest`` as for the constructor."""
        tok = text.replace("{", " { ").replace("}", " } ").split()
        names, parents, offsets, rotating, stack = [], [], [], [], []
        pending, pos = None, 0
        if "HIERARCHY" in tok:
            pos = tok.index("HIERARCHY") + 1
        try:
            while pos < len(tok) and tok[pos] != "MOTION":
                t = tok[pos]
                if t in ("ROOT", "JOINT"):
                    if (t == "ROOT") != (not stack):
                        raise ValueError("a ROOT inside a block, or a JOINT outside one")
                    pending, pos = tok[pos + 1], pos + 2
                elif t == "End" and tok[pos + 1] == "Site":
                    pending, pos = (names[stack[-1]] + "_end"), pos + 2
                elif t == "{":
                    if pending is None:
                        raise ValueError("'{' without a ROOT, JOINT or End Site line")
                    names.append(pending)
                    parents.append(stack[-1] if stack else -1)
                    offsets.append(None)
                    stack.append(len(names) - 1)
                    pending, pos = None, pos + 1
                elif t == "}":
                    stack.pop()
                    pos += 1
                elif t == "OFFSET":
                    offsets[stack[-1]] = [float(v) for v in tok[pos + 1:pos + 4]]
                    pos += 4
                elif t == "CHANNELS":
                    n = int(tok[pos + 1])
                    if any(c.lower().endswith("rotation") for c in tok[pos + 2:pos + 2 + n]):
                        rotating.append(stack[-1])
                    pos += 2 + n
                else:
                    raise ValueError(f"unexpected token {t!r}")
        except (IndexError, KeyError) as e:
            raise ValueError(f"from_bvh_header: malformed HIERARCHY block ({e})") from None
        if stack or not names or sum(p == -1 for p in parents) != 1 or any(o is None or len(o) != 3 for o in offsets):
            raise ValueError("from_bvh_header: unbalanced braces, no joint, more than one ROOT, or a joint without an OFFSET line")
        if joints is None:
            cj = rotating
        else:
            cj = [names.index(j) if isinstance(j, str) else int(j) for j in joints]
        return cls(parents, offsets, cj, rest=rest, names=names)


class _FkCall:
    """One checked ``joint_positions`` call: the device buffers and sizes both kernels take."""

    def __init__(self, src: torch.Tensor, skeleton: Skeleton, mean: torch.Tensor, std: torch.Tensor, kind: int, lens_dev, frames: int,
                 world_rotations: bool):
        self.sk, self.dev = skeleton, skeleton.to(src.device)
        self.mean, self.std, self.kind, self.lens_dev, self.frames, self.world_rotations = mean, std, kind, lens_dev, frames, world_rotations
        self.ld = int(src.shape[-1])
        self.rows = src.numel() // self.ld

    def _args(self, src):
        d = self.dev
        return (_stream_ptr(src.device), src.data_ptr(), self.ld, self.rows, self.kind, self.mean.data_ptr(), self.std.data_ptr(),
                self.sk.joints, self.sk.channels, d["parents"].data_ptr(), d["offsets"].data_ptr(), d["channel_joint"].data_ptr(),
                d["rest_rot"].data_ptr(), d["joint_channel"].data_ptr())

    def _tail(self):
        return (self.lens_dev.data_ptr() if self.lens_dev is not None else None, self.frames)

    def forward(self, src: torch.Tensor):
        J = self.sk.joints
        pos = torch.empty(src.shape[:-1] + (J, 3), device=src.device, dtype=torch.float32)
        wrot = torch.empty(src.shape[:-1] + (J, 3, 3), device=src.device, dtype=torch.float32) if self.world_rotations else None
        if self.rows == 0:              # an empty batch (a closed session that owes nothing): empty results, no call - an empty
            return pos, wrot            # tensor's pointer is null, which the C call refuses before it looks at the row count
        with torch.cuda.device(src.device):
            rc = _lib.lib().dsh_fk_positions(*self._args(src), pos.data_ptr(), 3 * J, wrot.data_ptr() if wrot is not None else None, 9 * J,
                                             *self._tail())
        _lib.check(rc, "dsh_fk_positions")
        return pos, wrot

    def vjp(self, src: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
        J, n = self.sk.joints, 3 * self.sk.channels
        g = g.to(torch.float32).contiguous()
        dx = torch.empty_like(src) if n == self.ld else torch.zeros_like(src)
        if self.rows == 0:
            return dx
        with torch.cuda.device(src.device):
            rc = _lib.lib().dsh_fk_positions_vjp(*self._args(src), g.data_ptr(), 3 * J, dx.data_ptr(), self.ld, *self._tail())
        _lib.check(rc, "dsh_fk_positions_vjp")
        return dx


class _JointPositions(torch.autograd.Function):
    """Forward: ``dsh_fk_positions``; backward: ``dsh_fk_positions_vjp`` on the input itself (the kernel recomputes the forward pass)."""

    @staticmethod
    def forward(ctx, src, call):
        pos, wrot = call.forward(src)
        ctx.call = call
        ctx.save_for_backward(src)
        if wrot is None:
            return pos
        ctx.mark_non_differentiable(wrot)
        return pos, wrot

    @staticmethod
    def backward(ctx, g_pos, *unused):
        (src,) = ctx.saved_tensors
        return ctx.call.vjp(src, g_pos), None


FK_KINDS = {"axis_angle": 0, "euler": 1}


def joint_positions(motion: torch.Tensor, skeleton: Skeleton, stats: PoseStats, *, split_pos: Optional[int] = None,
                    lengths: Optional[Sequence[int]] = None, kind: str = "axis_angle", world_rotations: bool = False):
    """World-space joint positions of the gesture channels, on the device (``dsh_fk_positions``): ``motion [..., C]`` standardised
    axis-angle triples (``kind="axis_angle"``, the sampler's representation) or standardised Euler 'XYZ' degrees (``kind="euler"``) ->
    ``[..., J, 3]``; with ``world_rotations=True`` also the joints' world rotation matrices ``[..., J, 3, 3]``, as a second result.
    Channel triple ``i`` is de-normalised with ``stats`` (the pair of the input kind) and drives joint ``skeleton.channel_joint[i]``; the
    other joints keep their rest rotation; the root sits at ``offsets[0]``.

    ``split_pos``: ``motion`` is the joint (gesture | expression) tensor and its first ``split_pos = 3 Jc`` channels are read in place.
    ``lengths`` (one frame count in ``1 .. T`` per clip of ``[..., T, C]``): frames behind a clip's length give exact zeros and are never
    read.  The result is differentiable with respect to ``motion`` for ``kind="axis_angle"`` (backward: ``dsh_fk_positions_vjp``;
    channels behind ``split_pos`` and padded frames get a zero gradient; the rotations carry none); ``kind="euler"`` is forward only and
    raises ``ValueError`` when a gradient is requested."""
    which = "joint_positions"
    if not isinstance(skeleton, Skeleton):
        raise ValueError(f"{which} needs a Skeleton, got {type(skeleton).__name__}")
    if not isinstance(stats, PoseStats):
        raise ValueError(f"{which} needs a PoseStats, got {type(stats).__name__}")
    if kind not in FK_KINDS:
        raise ValueError(f'{which}: kind must be "axis_angle" or "euler", got {kind!r}')
    if motion.dim() < 1:
        raise ValueError(f"{which} takes [..., channels] tensors")
    Cc = int(motion.shape[-1])
    n = Cc if split_pos is None else int(split_pos)
    if n != 3 * skeleton.channels or n > Cc:
        raise ValueError(f"{which}: {n} rotation channels of {Cc}, the skeleton drives {skeleton.channels} joints = {3 * skeleton.channels} channels")
    if stats.channels != n:
        raise ValueError(f"{which}: the statistics have {stats.channels} entries, the rotation channels are {n}")
    lens, T = None, 0
    if lengths is not None:
        if motion.dim() < 2:
            raise ValueError(f"{which}: lengths need a [..., T, channels] tensor")
        T = int(motion.shape[-2])
        lens = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        clips = motion.numel() // (T * Cc) if T * Cc else 0
        if len(lens) != clips or any(v < 1 or v > T for v in lens):
            raise ValueError(f"{which}: lengths needs one frame count in 1 .. {T} per clip ({clips}), got {lens}")
    wants_grad = motion.requires_grad and torch.is_grad_enabled()
    if wants_grad and kind == "euler":
        raise ValueError(f'{which}: kind="euler" is forward only; the gradient is built for kind="axis_angle"')
    if not motion.is_cuda:
        raise _lib.DshError(f"{which} runs on the GPU (no CPU fallback)")
    src = motion.to(torch.float32).contiguous()
    stats.to(src.device)
    mean, std = (stats.mean_axis_angle, stats.std_axis_angle) if kind == "axis_angle" else (stats.mean_euler, stats.std_euler)
    lens_dev = torch.tensor(lens, dtype=torch.int32).to(src.device) if lens is not None else None
    call = _FkCall(src, skeleton, mean, std, FK_KINDS[kind], lens_dev, T, bool(world_rotations))
    if wants_grad:
        return _JointPositions.apply(src, call)
    pos, wrot = call.forward(src)
    return (pos, wrot) if world_rotations else pos


def position_metrics(pos_a: torch.Tensor, pos_b: torch.Tensor, lengths: Optional[Sequence[int]] = None, *, pck_threshold: float):
    """MPJPE and position PCK of two sets of joint positions ``[..., T, J, 3]`` (or ``[..., J, 3]`` without ``lengths``), as 0-d device
    tensors ``{"mpjpe", "pck"}``: the mean joint distance, and the share of joints closer than ``pck_threshold`` (in the skeleton's
    units), over the valid frames.  ``lengths``: one frame count per clip; frames behind it count for nothing.  Plain torch on the
    tensors' device: no kernel of this library, no host synchronisation."""
    if pos_a.shape != pos_b.shape or pos_a.dim() < 2 or int(pos_a.shape[-1]) != 3:
        raise ValueError(f"position_metrics takes two [..., J, 3] tensors of one shape, got {tuple(pos_a.shape)} and {tuple(pos_b.shape)}")
    dist = (pos_a.to(torch.float32) - pos_b.to(torch.float32)).square().sum(-1).sqrt()          # [..., J]
    close = (dist < float(pck_threshold)).to(torch.float32)
    if lengths is None:
        return {"mpjpe": dist.mean(), "pck": close.mean()}
    if pos_a.dim() < 3:
        raise ValueError("position_metrics: lengths need [..., T, J, 3] tensors")
    T, J = int(pos_a.shape[-3]), int(pos_a.shape[-2])
    lens = lengths if isinstance(lengths, torch.Tensor) else torch.tensor([int(v) for v in lengths])
    lens = lens.to(device=dist.device, dtype=torch.int64).reshape(-1)
    if lens.numel() * T * J != dist.numel():
        raise ValueError(f"position_metrics: lengths needs one frame count per clip ({dist.numel() // max(T * J, 1)}), got {lens.numel()}")
    valid = (torch.arange(T, device=dist.device).view(1, T) < lens.view(-1, 1)).view(-1, T, 1)
    count = (valid.sum() * J).clamp_min(1).to(torch.float32)
    zero = torch.zeros((), device=dist.device)
    return {"mpjpe": torch.where(valid, dist.view(-1, T, J), zero).sum() / count,
            "pck": torch.where(valid, close.view(-1, T, J), zero).sum() / count}


def guidance_grad_torch(z: torch.Tensor, target, weight, vel, acc, lengths=None, scale: float = 1.0) -> torch.Tensor:
    """``g = scale * d log p / d z`` of the guidance energy (:class:`MotionGuidance`) in plain torch, in ``z``'s dtype, on ``z``'s device:
    the five-point stencil the step kernels evaluate, in their operation order.  ``z [B, T, C]``; ``target`` / ``weight`` ``[B, T, C]`` or
    None; ``vel`` / ``acc`` ``[C]`` or None; ``lengths``: one frame count per clip or None."""
    B, T, Cc = z.shape
    t = torch.arange(T, device=z.device).view(1, T, 1)
    L = torch.full((B, 1, 1), T, device=z.device) if lengths is None else \
        torch.as_tensor(lengths, device=z.device).to(torch.int64).clamp(0, T).view(B, 1, 1)
    zero = torch.zeros((), dtype=z.dtype, device=z.device)
    pad = torch.zeros(B, 1, Cc, dtype=z.dtype, device=z.device)

    def shift(u, k):        # u[t + k], zeros outside
        if k == 0:
            return u
        fill = pad.expand(B, min(abs(k), T), Cc)
        return torch.cat([u[:, k:], fill], 1) if k > 0 else torch.cat([fill, u[:, :k]], 1)

    total = torch.zeros_like(z)
    if weight is not None:
        y = zero if target is None else target.to(device=z.device, dtype=z.dtype)
        total = weight.to(device=z.device, dtype=z.dtype) * (z - y)
    if vel is not None:
        v = torch.where(t <= L - 2, shift(z, 1) - z, zero)                      # v[t] = z[t+1] - z[t], t = 0 .. L-2
        total = total + vel.to(device=z.device, dtype=z.dtype).view(1, 1, Cc) * (shift(v, -1) - v)
    if acc is not None:
        a = torch.where((t >= 1) & (t <= L - 2), (shift(z, 1) - 2 * z) + shift(z, -1), zero)      # a[t], t = 1 .. L-2
        total = total + acc.to(device=z.device, dtype=z.dtype).view(1, 1, Cc) * ((shift(a, -1) - 2 * a) + shift(a, 1))
    return torch.where(t < L, -(scale * total), zero)


class MotionGuidance:
    """Soft constraints for the sampling loops: a closed family of per-column quadratic energies, handed to ``ddim_sample_loop`` /
    ``p_sample_loop`` as ``cond_fn=`` or to the trainer's entry points as ``guidance=``.  With ``L`` the clip's length and ``z`` the guided
    signal of column ``c`` of clip ``b``::

        log p(y | z) = -1/2 sum_t W[b,t,c] (z[t] - Y[b,t,c])^2          attraction (keyframes / soft targets)
                       -1/2 vel[c] sum_{t=0..L-2} (z[t+1] - z[t])^2      velocity damping
                       -1/2 acc[c] sum_{t=1..L-2} (z[t+1] - 2 z[t] + z[t-1])^2      acceleration (jitter) damping

    and every denoise step uses ``s_k * d log p / d z`` where the reference uses the value of its ``cond_fn``, fused into the step kernel.
    ``target`` = Y and ``weight`` = W >= 0 are fp32 ``[B, T, C]`` tensors (``weight=None`` with a target: 1 everywhere); ``vel`` / ``acc``
    fp32 ``[C]``; all on one device.  ``space="x_t"``: z is the noisy sample — exactly the reference's ``cond_fn(x, t)`` contract.
    ``space="x0"`` (default): z is the step's ``pred_xstart``; the denoiser's Jacobian is not applied.  ``level_scale``: one factor per
    level of the run (``respacing`` entries for the DDIM loops, ``diffusion_steps`` for the DDPM loop; None: 1); a level with factor 0 runs
    unguided.  No term couples columns.

    The object is also the reference's hook itself: ``g(x, t, **model_kwargs)`` returns the gradient for ``space="x_t"`` in plain torch
    on any device (``t``: the ORIGINAL timesteps a SpacedDiffusion passes; set ``timestep_map`` to the run's map when ``level_scale`` is
    given; ``length`` in ``model_kwargs`` gives the clips' lengths).  For ``space="x0"`` the call raises: the contract has no pred_xstart."""

    def __init__(self, target=None, weight=None, vel=None, acc=None, space: str = "x0", level_scale=None, timestep_map=None):
        if space not in _lib.GUIDE_SPACES:
            raise ValueError(f'space must be "x_t" or "x0", got {space!r}')
        if weight is not None and target is None:
            raise ValueError("weight needs a target")
        tensors = [(n, v) for n, v in (("target", target), ("weight", weight), ("vel", vel), ("acc", acc)) if v is not None]
        for n, v in tensors:
            if not isinstance(v, torch.Tensor) or v.dtype != torch.float32:
                raise ValueError(f"MotionGuidance: {n} must be a float32 tensor")
            if v.device != tensors[0][1].device:
                raise ValueError(f"MotionGuidance: {n} is on {v.device}, {tensors[0][0]} on {tensors[0][1].device}")
        if target is not None:
            if target.dim() != 3:
                raise ValueError(f"MotionGuidance: target must be [B, T, C], got {tuple(target.shape)}")
            if weight is None:
                weight = torch.ones_like(target)
            if weight.shape != target.shape:
                raise ValueError(f"MotionGuidance: weight {tuple(weight.shape)} differs from target {tuple(target.shape)}")
            if bool((weight < 0).any()):
                raise ValueError("MotionGuidance: weight must be >= 0")
        cols = None if target is None else int(target.shape[2])
        for n, v in (("vel", vel), ("acc", acc)):
            if v is None:
                continue
            if v.dim() != 1 or (cols is not None and int(v.shape[0]) != cols):
                raise ValueError(f"MotionGuidance: {n} must be [C]{'' if cols is None else f' = [{cols}]'}, got {tuple(v.shape)}")
            cols = int(v.shape[0])
        self.target = None if target is None else target.contiguous()
        self.weight = None if weight is None else weight.contiguous()
        self.vel = None if vel is None else vel.contiguous()
        self.acc = None if acc is None else acc.contiguous()
        self.space = space
        self.level_scale = None if level_scale is None else [float(v) for v in level_scale]
        self.timestep_map = None if timestep_map is None else [int(v) for v in timestep_map]

    @property
    def channels(self) -> Optional[int]:
        for v in (self.target, self.vel, self.acc):
            if v is not None:
                return int(v.shape[-1])
        return None

    def with_terms(self, target, weight) -> "MotionGuidance":
        """The same guidance with another ``target`` / ``weight`` pair (a window of a longer stream)."""
        if target.shape != weight.shape or target.dim() != 3 or int(target.shape[2]) != self.channels:
            raise ValueError(f"with_terms: target {tuple(target.shape)} / weight {tuple(weight.shape)} must be [B, T, {self.channels}]")
        g = copy.copy(self)              # (slices of tensors this object has validated: no second look at their values, no host sync)
        g.target, g.weight = target.contiguous(), weight.contiguous()
        return g

    @classmethod
    def from_keyframes(cls, poses, frames, columns, weight, B: int, T: int, C: int, device="cuda", **kw) -> "MotionGuidance":
        """Keyframes as soft targets: ``poses [K, n]`` (every row of the batch) or ``[B, K, n]`` holds the standardised values of the ``n``
        columns covered by ``columns`` (half-open ``(lo, hi)`` ranges, in order) at the ``K`` frame indices ``frames``; ``weight``: one
        float, or one per keyframe ``[K]``.  Builds ``target`` / ``weight`` ``[B, T, C]`` on ``device`` (0 off the keyframes); ``kw`` goes
        to the constructor (``vel=``, ``acc=``, ``space=``, ``level_scale=``)."""
        B, T, C = int(B), int(T), int(C)
        fr = [int(f) for f in frames]
        if not fr or any(f < 0 or f >= T for f in fr) or len(set(fr)) != len(fr):
            raise ValueError(f"from_keyframes: frames must be distinct indices in 0 .. {T - 1}, got {fr}")
        cols = [c for lo, hi in _ranges(columns, "column", C) for c in range(lo, hi)]
        if not cols or len(set(cols)) != len(cols):
            raise ValueError("from_keyframes: the column ranges must be non-empty and disjoint")
        p = torch.as_tensor(poses, dtype=torch.float32)
        if p.dim() == 2:
            p = p.unsqueeze(0).expand(B, -1, -1)
        if tuple(p.shape) != (B, len(fr), len(cols)):
            raise ValueError(f"from_keyframes: poses must be [K, n] or [B, K, n] = {(B, len(fr), len(cols))}, got {tuple(p.shape)}")
        w = torch.as_tensor(weight, dtype=torch.float32).reshape(-1)
        if w.numel() not in (1, len(fr)) or bool((w < 0).any()):
            raise ValueError(f"from_keyframes: weight must be one value >= 0 or one per keyframe ({len(fr)})")
        dev = torch.device(device)
        fi = torch.tensor(fr, device=dev).view(-1, 1)
        ci = torch.tensor(cols, device=dev).view(1, -1)
        Y = torch.zeros(B, T, C, device=dev)
        W = torch.zeros(B, T, C, device=dev)
        Y[:, fi, ci] = p.to(dev)
        W[:, fi, ci] = w.to(dev).expand(len(fr)).view(1, -1, 1).expand(B, len(fr), len(cols))
        return cls(Y, W, **kw)

    def scale_at(self, t) -> float:
        """The level factor at the ORIGINAL timestep ``t`` (the timestep itself is the level without a ``timestep_map``)."""
        if self.level_scale is None:
            return 1.0
        k = int(t) if self.timestep_map is None else self.timestep_map.index(int(t))
        return self.level_scale[k]

    def __call__(self, x, t, **kwargs):
        if self.space != "x_t":
            raise TypeError('MotionGuidance(space="x0") is not a cond_fn(x, t): the contract carries no pred_xstart')
        ts = set(int(v) for v in t.reshape(-1).tolist()) if isinstance(t, torch.Tensor) else {int(t)}
        if len(ts) != 1:
            raise NotImplementedError("one timestep per call")
        length = kwargs.get("length")
        lens = None if length is None else [int(v) for v in (length.tolist() if isinstance(length, torch.Tensor) else length)]
        return guidance_grad_torch(x, self.target, self.weight, self.vel, self.acc, lens, self.scale_at(ts.pop()))


def _gain_row(gain, steps: int, what: str) -> np.ndarray:
    """One encoder's gains as float32 ``[steps]``: ``None`` (1 everywhere), a number, an array of ``steps`` values, or a callable
    ``t -> gain`` evaluated here, on the host, at every original timestep."""
    if gain is None:
        row = np.ones(steps, dtype=np.float32)
    elif callable(gain):
        row = np.asarray([float(gain(t)) for t in range(steps)], dtype=np.float32)
    else:
        try:
            a = np.asarray(gain.detach().cpu().numpy() if isinstance(gain, torch.Tensor) else gain, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"CFGSchedule: {what} must be None, a number, {steps} values or a callable t -> gain") from e
        if a.ndim == 0:
            a = np.full(steps, float(a))
        if a.shape != (steps,):
            raise ValueError(f"CFGSchedule: {what} needs one gain per original timestep ({steps}), got shape {a.shape}")
        with np.errstate(over="ignore"):
            row = a.astype(np.float32)
    if not np.all(np.isfinite(row)):
        raise ValueError(f"CFGSchedule: the {what} gains must be finite (in float32)")
    return row


class CFGSchedule:
    """How strongly the classifier-free guidance acts, per model timestep and per encoder, and the std rescale of the guided prediction
    (``dsh_set_guidance_schedule``).  At a clip's original timestep ``t`` encoder ``m`` mixes with

        ``s_eff = 1 + gain_m[t] * (cond_scale - 1)``      (``gain == 1``: ``cond_scale`` itself; ``gain == 0``: the conditional prediction)

    so a gain shapes the part of the scale that guides and leaves ``cond_scale`` (one value or one per clip) the knob it was.  ``rescale``
    (φ in ``[0, 1]``, one value or an ``(expression, gesture)`` pair) pulls the std of each clip's guided eps back towards the conditional
    prediction's: ``eps *= φ * std(k) / std(eps) + (1 - φ)`` over the clip's own frames and the encoder's columns (Lin et al.,
    "Common diffusion noise schedules and sample steps are flawed", ``guidance_rescale``).

    ``expression`` / ``gesture``: ``None`` (gain 1), a float, ``steps`` values, or a callable ``t -> gain`` evaluated on the host.
    Give it to ``UniDiffuser.set_guidance_schedule`` (sticky) or as ``cfg_schedule=`` to a sampling loop (that call only).  Not to be
    confused with :class:`MotionGuidance`, the soft constraints on the motion itself."""

    def __init__(self, expression=None, gesture=None, rescale=0.0, steps: int = 1000):
        if not isinstance(steps, (int, np.integer)) or int(steps) < 1:
            raise ValueError(f"CFGSchedule: steps must be a positive integer, got {steps!r}")
        self.steps = int(steps)
        self.expression = _gain_row(expression, self.steps, "expression")
        self.gesture = _gain_row(gesture, self.steps, "gesture")
        try:
            phi = np.asarray(rescale, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError) as e:
            raise ValueError("CFGSchedule: rescale must be one number or an (expression, gesture) pair") from e
        if phi.size not in (1, 2):
            raise ValueError(f"CFGSchedule: rescale must be one number or an (expression, gesture) pair, got {phi.size} values")
        phi = np.broadcast_to(phi, (2,)).astype(np.float32)
        if not np.all(np.isfinite(phi)) or np.any(phi < 0) or np.any(phi > 1):
            raise ValueError(f"CFGSchedule: rescale must lie in [0, 1], got {rescale!r}")
        self.rescale = (float(phi[0]), float(phi[1]))         # (float32-representable: what the kernels read)

    @classmethod
    def interval(cls, t_lo: int, t_hi: int, rescale=0.0, steps: int = 1000) -> "CFGSchedule":
        """The guidance interval: gain 1 at the original timesteps ``t_lo <= t <= t_hi``, 0 outside, for both encoders."""
        t_lo, t_hi = int(t_lo), int(t_hi)
        if not 0 <= t_lo <= t_hi < int(steps):
            raise ValueError(f"CFGSchedule.interval: needs 0 <= t_lo <= t_hi < {steps}, got ({t_lo}, {t_hi})")
        row = np.zeros(int(steps), dtype=np.float32)
        row[t_lo:t_hi + 1] = 1.0
        return cls(row, row.copy(), rescale, steps)

    @classmethod
    def from_levels(cls, diffusion, gains, gesture_gains=None, rescale=0.0) -> "CFGSchedule":
        """One gain per spaced level of ``diffusion`` (a ``'ddimK'`` / ``'logsnrK'`` SpacedDiffusion; level 0 is the last step), for both
        encoders or, with ``gesture_gains``, ``gains`` for the expression encoder.  The levels map through ``diffusion.timestep_map``, and
        an original timestep takes the gain of the smallest kept timestep >= it (above the largest: the top level's), so a restart or a
        plain evaluation between two levels finds the gain of the level above."""
        tmap = np.asarray(sorted(int(v) for v in diffusion.timestep_map), dtype=np.int64)
        steps = int(getattr(diffusion, "original_num_steps", len(tmap)))
        idx = np.minimum(np.searchsorted(tmap, np.arange(steps), side="left"), len(tmap) - 1)

        def row(g, what):
            a = np.asarray(g, dtype=np.float64)
            if a.shape != (len(tmap),):
                raise ValueError(f"CFGSchedule.from_levels: {what} needs one gain per level ({len(tmap)}), got shape {a.shape}")
            return a[idx]
        e = row(gains, "gains")
        return cls(e, e if gesture_gains is None else row(gesture_gains, "gesture_gains"), rescale, steps)

    @property
    def trivial(self) -> bool:
        """All gains 1 and no rescale: the unscheduled arithmetic."""
        return bool(np.all(self.expression == 1) and np.all(self.gesture == 1) and self.rescale == (0.0, 0.0))

    @property
    def same_for_both(self) -> bool:
        return bool(np.array_equal(self.expression, self.gesture) and self.rescale[0] == self.rescale[1])

    def __eq__(self, other):
        return (isinstance(other, CFGSchedule) and self.steps == other.steps and self.rescale == other.rescale
                and np.array_equal(self.expression, other.expression) and np.array_equal(self.gesture, other.gesture))

    __hash__ = None


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
