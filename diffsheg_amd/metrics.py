"""Validation metrics of the reference's validation loop (trainers/ddpm_show_trainer.py:440-583, ddpm_beat_trainer.py:489-644) on the
device: the FGD pose encoder (``HalfEmbeddingNet``, models/motion_autoencoder.py:192-204), MSE / PCK / diversity of a batch, the
``AverageMeter`` and the Frechet distance.

    latents  = eval_model(outputs)                        # [B, 300], device
    m        = batch_metrics(outputs, motions, joint_dim) # device scalars, no sync
    fgd      = frechet_distance(latents_out, latents_ori) # host, float64, numpy only

The encoder and the batch metrics are HIP kernels (csrc/pose_encoder.hip, csrc/metrics.hip); there is no torch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .weights import fid_dims, strip_ddp_prefix

DIVERSITY_GROUP = 50      # "In Ye et al. (ECCV'22), Batch size is 50 when evaluating diversity" (ddpm_show_trainer.py:531)


class HalfEmbeddingNet:
    """``HalfEmbeddingNet(args).eval()`` of the reference with the weights of ``state_dict`` (its own key names; a ``module.`` prefix
    is stripped): ``latents = eval_model(x)`` for ``x [B, frames >= n_poses, net_dim_pose]`` gives ``mu`` of the first ``n_poses``
    frames of every clip, ``[B, vae_length]`` fp32 on the device, asynchronously.  ``cfg_or_opt`` supplies ``n_poses``,
    ``net_dim_pose`` and (optionally; default 300) ``vae_length``."""

    def __init__(self, cfg_or_opt, state_dict: Dict[str, torch.Tensor], device="cuda:0"):
        if not torch.cuda.is_available():
            raise _lib.DshError("no GPU visible: diffsheg_amd has no CPU fallback")
        self.n_poses, self.dim, self.vae_length = fid_dims(cfg_or_opt)
        self.device = torch.device(device)
        self._lib = _lib.lib()
        torch.cuda.set_device(self.device)
        self._stream = torch.cuda.current_stream(self.device)
        self._h = create_fgd_handle(self.n_poses, self.dim, self.vae_length, self._stream.cuda_stream)
        load_fgd_weights(self._h, state_dict)
        _lib.check(self._lib.dsh_fgd_finalize(self._h), "dsh_fgd_finalize")

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 3 or int(x.shape[2]) != self.dim:
            raise ValueError(f"HalfEmbeddingNet takes [B, frames, {self.dim}], got {tuple(x.shape)}")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        B, frames = int(x.shape[0]), int(x.shape[1])
        out = torch.empty(B, self.vae_length, device=self.device, dtype=torch.float32)
        cur = torch.cuda.current_stream(self.device)
        if cur != self._stream:
            self._stream.wait_stream(cur)
        _lib.check(self._lib.dsh_fgd_encode(self._h, x.data_ptr(), B, frames, out.data_ptr()), "dsh_fgd_encode")
        if cur != self._stream:
            cur.wait_stream(self._stream)
            x.record_stream(self._stream)
            out.record_stream(self._stream)
        return out

    forward = __call__

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dsh_fgd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def create_fgd_handle(n_poses: int, dim: int, vae_length: int, stream: int = 0) -> C.c_void_p:
    h = C.c_void_p()
    _lib.check(_lib.lib().dsh_fgd_create(n_poses, dim, vae_length, C.c_void_p(stream), C.byref(h)), "dsh_fgd_create")
    return h


def load_fgd_weights(h: C.c_void_p, state_dict: Dict[str, torch.Tensor]) -> None:
    """Every floating-point tensor of a ``HalfEmbeddingNet`` state dict into the handle, by key name (host side; needs no device)."""
    L = _lib.lib()
    for name, t in strip_ddp_prefix(state_dict).items():
        if not torch.is_floating_point(t):
            continue                      # num_batches_tracked
        a = t.detach().to("cpu", torch.float32).contiguous()
        shape = (C.c_int64 * max(a.dim(), 1))(*a.shape)
        _lib.check(L.dsh_fgd_load_tensor(h, name.encode(), C.c_void_p(a.data_ptr()), shape, a.dim()), f"dsh_fgd_load_tensor({name})")


def packed_fgd_layers(h: C.c_void_p):
    """Test helper (host only): the layers exactly as ``dsh_fgd_finalize`` would upload them — a list of ``(W [N, K padded], bias [N],
    K)`` float32 arrays: BatchNorm folded, conv taps repacked to ``[out, k * in]``, the first Linear's columns permuted to the
    channels-last flatten, K zero padded to 32.  Layers 0 .. 3 are the convolutions, then the ``out_net`` Linears, ``fc_mu`` last."""
    L = _lib.lib()
    out = []
    for i in range(int(L.dsh_fgd_debug_num_layers(h))):
        dims = (C.c_int32 * 3)()
        _lib.check(L.dsh_fgd_debug_packed_layer(h, i, dims, None, None), "dsh_fgd_debug_packed_layer")
        N, K, Kp = int(dims[0]), int(dims[1]), int(dims[2])
        W = np.empty((N, Kp), dtype=np.float32)
        b = np.empty((N,), dtype=np.float32)
        _lib.check(L.dsh_fgd_debug_packed_layer(h, i, dims, W.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)),
                   "dsh_fgd_debug_packed_layer")
        out.append((W, b, K))
    return out


def diversity_groups(B: int):
    """``(b_div, n_groups)`` of a batch of ``B`` clips: groups of ``min(50, B)`` consecutive clips, the incomplete last group dropped
    (ddpm_show_trainer.py:531-545).  ``B = 1`` is refused: the reference divides by ``b_div (b_div - 1) = 0`` there."""
    B = int(B)
    if B < 2:
        raise ValueError("diversity needs at least two clips per batch (the reference divides by B_div (B_div - 1))")
    b_div = min(DIVERSITY_GROUP, B)
    return b_div, B // b_div


def batch_metrics(outputs: torch.Tensor, motions: torch.Tensor, joint_dim: int) -> Dict[str, torch.Tensor]:
    """MSE, PCK and diversity of one validation batch on the device (``dsh_op_batch_metrics``; three launches, no sync).
    ``outputs`` / ``motions`` ``[B, T, C]``; ``joint_dim`` 1 (SHOW: PCK per element) or 3 (BEAT: per joint triplet).  Returns device
    tensors: ``"mse"``, ``"pck"`` (float64 scalars), ``"sq_sum"`` (float64), ``"pck_count"`` (int64), ``"diversity"`` (float64, one
    value per complete group of ``b_div`` clips) and the host ints ``"b_div"``, ``"batch"``."""
    if outputs.shape != motions.shape or outputs.dim() != 3:
        raise ValueError(f"batch_metrics takes two [B, T, C] tensors, got {tuple(outputs.shape)} and {tuple(motions.shape)}")
    if not outputs.is_cuda:
        raise _lib.DshError("batch_metrics runs on the GPU: there is no CPU fallback")
    B, T, Cc = (int(v) for v in outputs.shape)
    b_div, groups = diversity_groups(B)
    o = outputs.to(torch.float32).contiguous()
    m = motions.to(device=o.device, dtype=torch.float32).contiguous()
    L = _lib.lib()
    nbytes = int(L.dsh_batch_metrics_result_bytes(B, T, Cc, b_div))
    res = torch.empty(nbytes // 8, dtype=torch.float64, device=o.device)
    stream = torch.cuda.current_stream(o.device).cuda_stream
    _lib.check(L.dsh_op_batch_metrics(C.c_void_p(stream), o.data_ptr(), m.data_ptr(), B, T, Cc, int(joint_dim), b_div, res.data_ptr()),
               "dsh_op_batch_metrics")
    H = _lib.METRICS_HEADER
    return {"sq_sum": res[0], "pck_count": res[1:2].view(torch.int64)[0], "mse": res[2], "pck": res[3],
            "diversity": res[H:H + groups], "b_div": b_div, "batch": B}


class AverageMeter:
    """The reference's meter (ddpm_show_trainer.py:1197-1227): ``sum += val * n``, ``count += n``; ``all_reduce`` sums
    ``[sum, count]`` as a float32 tensor over the ranks."""

    def __init__(self, name: str = ""):
        self.name = name
        self.reset()

    def reset(self) -> None:
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n: int = 1) -> None:
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count

    def all_reduce(self, group=None, device: Optional[torch.device] = None) -> None:
        import torch.distributed as dist
        if device is None:
            device = torch.device("cuda") if dist.get_backend(group) == "nccl" else torch.device("cpu")
        total = torch.tensor([self.sum, self.count], dtype=torch.float32, device=device)
        dist.all_reduce(total, dist.ReduceOp.SUM, group=group)
        self.sum, self.count = total.tolist()
        self.avg = self.sum / self.count


def activation_statistics(x):
    """``mu = mean``, ``sigma = np.cov(rowvar=False)`` in float64 (datasets/data_tools.py:416-482, utils/metrics.py:60-70)."""
    x = np.asarray(x, dtype=np.float64)
    return x.mean(axis=0), np.atleast_2d(np.cov(x, rowvar=False))


def _sqrt_psd(s: np.ndarray) -> np.ndarray:
    w, v = np.linalg.eigh((s + s.T) * 0.5)
    return (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T


def frechet_distance(a, b) -> float:
    """``d^2 = |mu1 - mu2|^2 + Tr s1 + Tr s2 - 2 Tr sqrtm(s1 s2)`` between the Gaussians fitted to the rows of ``a`` and ``b``
    (``[N, D]`` latents), float64, numpy only.  ``s1 s2`` is similar to the symmetric PSD matrix ``s1^1/2 s2 s1^1/2``, so
    ``Tr sqrtm(s1 s2) = sum sqrt(eig(s1^1/2 s2 s1^1/2))``: two ``eigh``, negative eigenvalues (round-off of singular covariances,
    N < D) clipped to 0 — where the reference's ``scipy.linalg.sqrtm`` takes a Schur decomposition of the non-symmetric product."""
    mu1, s1 = activation_statistics(a)
    mu2, s2 = activation_statistics(b)
    r = _sqrt_psd(s1)
    m = r @ s2 @ r
    w = np.linalg.eigvalsh((m + m.T) * 0.5)
    tr_covmean = float(np.sqrt(np.clip(w, 0.0, None)).sum())
    diff = mu1 - mu2
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2.0 * tr_covmean)
