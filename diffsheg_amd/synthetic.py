"""Seeded synthetic conditioning.  There are no datasets / HuBERT weights offline,
so tests, fixtures and bench all draw inputs of the reference's shapes from CPU generators:

    audio_emb (mel)            ~ N(0,1)  [B,T,128]      datasets/show.py:65-144
    pretrain_aud_feat (HuBERT) ~ N(0,1)  [B,T,1024]
    person_id                  one-hot   [B,S]   row i -> i mod S
    x_T                        ~ N(0,1)  [B,T,C]

CPU ``torch.Generator`` streams are bit-reproducible across machines running the same torch
build, so fixtures store only seeds + expected outputs.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .config import DiffSHEGConfig

_TORCH_RANDN = torch.randn     # bound at import: the fixture generator monkey-patches torch.randn


def make_inputs(cfg: DiffSHEGConfig, batch: int, frames: Optional[int] = None, seed: int = 3) -> Dict[str, torch.Tensor]:
    T = cfg.n_poses if frames is None else frames
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    audio = torch.randn(batch, T, cfg.audio_dim, generator=g)
    hubert = torch.randn(batch, T, cfg.hubert_dim, generator=g)
    x_t = torch.randn(batch, T, cfg.net_dim_pose, generator=g)
    pid = torch.zeros(batch, cfg.style_dim)
    pid[torch.arange(batch), torch.arange(batch) % cfg.style_dim] = 1.0
    return {"audio_emb": audio, "pretrain_aud_feat": hubert, "person_id": pid, "x_T": x_t}


class SeededNoise:
    """Gaussian draws in the reference's draw order from a seeded CPU generator.

    ``randn(shape)`` returns a CPU fp32 tensor; the product sampler uploads it, the fixture
    generator monkey-patches the reference's ``th.randn`` / ``th.randn_like`` with it.
    """

    def __init__(self, seed: int):
        self.gen = torch.Generator(device="cpu")
        self.gen.manual_seed(seed)
        self.count = 0

    def randn(self, shape) -> torch.Tensor:
        self.count += 1
        return _TORCH_RANDN(*tuple(shape), generator=self.gen)


def make_motion_pair(cfg, batch: int, seed: int, frames: int | None = None):
    """Two related standardised-motion batches ``[batch, frames, net_dim_pose]`` (CPU fp32) for the validation-metric tests:
    ``motions = x`` ~ N(0, 1) and ``outputs = 0.8 x + 0.3 noise``, so that MSE, PCK (neither 0 nor 1), diversity and the Frechet
    distance of their latents are all non-trivial.  Returns ``(outputs, motions)``."""
    T = int(frames if frames is not None else cfg.n_poses)
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    x = torch.randn(batch, T, cfg.net_dim_pose, generator=g)
    n = torch.randn(batch, T, cfg.net_dim_pose, generator=g)
    return (0.8 * x + 0.3 * n).contiguous(), x.contiguous()


# ---- rotation fixtures (tests/golden/rotations_beat.npz): inputs and statistics regenerated from seeds ------------------------------
def make_pose_stat_vectors(joints: int, seed: int) -> Dict[str, torch.Tensor]:
    """Synthetic BEAT pose statistics ``[3 J]`` (CPU fp32): ``mean_axis_angle`` ~ N(0, 0.2) rad, ``std_axis_angle`` ~ U(0.05, 0.5) rad,
    ``mean_euler`` ~ N(0, 15) degrees, ``std_euler`` ~ U(3, 30) degrees; keyword arguments of :class:`diffsheg_amd.glue.PoseStats`."""
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    n = 3 * int(joints)
    return {"mean_axis_angle": 0.2 * torch.randn(n, generator=g), "std_axis_angle": 0.05 + 0.45 * torch.rand(n, generator=g),
            "mean_euler": 15.0 * torch.randn(n, generator=g), "std_euler": 3.0 + 27.0 * torch.rand(n, generator=g)}


def make_rotation_inputs(batch: int, frames: int, joints: int, seed: int):
    """Standardised inputs ~ N(0, 1), ``[batch, frames, 3 J]`` CPU fp32: ``(axis_angle, euler)`` for the two directions."""
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    return torch.randn(batch, frames, 3 * joints, generator=g), torch.randn(batch, frames, 3 * joints, generator=g)


# Euler 'XYZ' degrees of the forward edge block's gimbal joints: six with the middle angle within 0.5 degrees of +-90 (cos Y still above
# fp32 rounding, so the rotation is determined), then two exactly on it (cos Y = 0: only Y and X -+ Z are determined in any fp32 run)
_GIMBAL_EULER = ((10.0, 89.7, 20.0), (-35.0, -89.8, 50.0), (70.0, 89.55, -160.0), (120.0, -89.6, -30.0), (15.0, 89.95, -100.0),
                 (-60.0, -89.9, 5.0), (0.0, 90.0, 0.0), (120.0, -90.0, -30.0))
# Euler 'XYZ' degrees of the inverse edge block: zero, the small-angle branch, |Y| = 89.9, half turns (quaternion w ~ 0)
_INVERSE_EDGE_EULER = ((0.0, 0.0, 0.0), (1e-5, 0.0, 0.0), (30.0, 89.9, -40.0), (-20.0, -89.9, 10.0), (180.0, 0.0, 0.0),
                       (179.95, 0.02, -0.03), (0.0, 0.0, -180.0), (100.0, 0.0, 180.0), (0.0, 179.0, 0.0), (45.0, -30.0, 170.0))


def _axis_angle_of_euler_xyz(deg) -> torch.Tensor:
    """float64 axis-angle vector of Rx(a) Ry(b) Rz(c) by the quaternion product of the three axis rotations (angle in [0, 2 pi))."""
    import math
    a, b, c = (math.radians(v) / 2 for v in deg)
    qx, qy, qz = (math.cos(a), math.sin(a), 0.0, 0.0), (math.cos(b), 0.0, math.sin(b), 0.0), (math.cos(c), 0.0, 0.0, math.sin(c))

    def mul(p, q):
        return (p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3], p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2],
                p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1], p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0])
    w, x, y, z = mul(mul(qx, qy), qz)
    n = math.sqrt(x * x + y * y + z * z)
    ang = 2.0 * math.atan2(n, w)
    return torch.tensor([x / n * ang, y / n * ang, z / n * ang] if n > 0 else [0.0, 0.0, 0.0], dtype=torch.float64)


def make_rotation_edge_cases() -> Dict[str, torch.Tensor]:
    """The edge block of the rotation fixture, for statistics of mean 0 / std 1 (CPU fp32, ``[1, 1, 3 J]``).

    ``axis_angle`` (14 joints): the zero vector; ``|v|`` = 5e-7 and 2e-6 (either side of the small-angle threshold 1e-6); angles
    pi - 1e-3, pi + 0.5 and 2 pi - 0.1; six joints whose middle Euler angle is within 0.5 degrees of +-90 and two exactly on it
    (``_GIMBAL_EULER``).
    ``euler`` (10 joints, degrees): ``_INVERSE_EDGE_EULER``."""
    import math
    ax1 = torch.tensor([0.6, 0.0, 0.8], dtype=torch.float64)
    ax2 = torch.tensor([1.0, -2.0, 2.0], dtype=torch.float64) / 3.0
    rows = [torch.zeros(3, dtype=torch.float64), ax1 * 5e-7, ax2 * 2e-6, ax2 * (math.pi - 1e-3), ax1 * (math.pi + 0.5),
            ax2 * (2 * math.pi - 0.1)] + [_axis_angle_of_euler_xyz(e) for e in _GIMBAL_EULER]
    aa = torch.stack(rows).to(torch.float32).reshape(1, 1, -1)
    eu = torch.tensor(_INVERSE_EDGE_EULER, dtype=torch.float64).to(torch.float32).reshape(1, 1, -1)
    return {"axis_angle": aa, "euler": eu}
