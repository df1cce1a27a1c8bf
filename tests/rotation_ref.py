"""float64 numpy restatement of the two BEAT rotation chains, used only by tests.

Forward (trainers/ddpm_beat_trainer.py:1056-1060 on datasets/rotation_converter.py): de-normalise, axis-angle -> unit quaternion
(:204-233: sin(a/2)/a, with 1/2 - a^2/48 below 1e-6) -> rotation matrix (:251-280) -> Euler 'XYZ' (:342-381: for R = Rx(X) Ry(Y) Rz(Z),
R02 = sin Y, (R12, R22) = (-sin X, cos X) cos Y, (R01, R00) = (-sin Z, cos Z) cos Y) -> degrees -> normalise.
Inverse (datasets/beat.py:380-383, :401): de-normalise, degrees -> radians -> Rx Ry Rz (:147-173) -> quaternion from the matrix
(:44-103: four |q| components from the diagonal, the candidate built on the largest, denominator floored at 0.1) -> axis-angle
(:12-40: half angle atan2(|xyz|, w), which exceeds pi / 2 for w < 0) -> normalise.

Also the helpers the comparisons need: rotation matrices from Euler degrees and from axis-angle vectors (Rodrigues, independent of the
quaternion route), angle differences modulo 360, and the fixture's two conditioning masks."""
from __future__ import annotations

import numpy as np

SMALL = 1e-6


def _sin_half_over_angle(half, angle):
    safe = np.where(np.abs(angle) < SMALL, 1.0, angle)
    return np.where(np.abs(angle) < SMALL, 0.5 - angle * angle / 48.0, np.sin(half) / safe)


def axis_angle_to_euler_deg(v: np.ndarray) -> np.ndarray:
    """[..., 3] axis-angle vectors (rad) -> [..., 3] Euler 'XYZ' degrees, float64."""
    v = np.asarray(v, dtype=np.float64)
    angle = np.sqrt((v * v).sum(-1))
    half = 0.5 * angle
    k = _sin_half_over_angle(half, angle)
    r, i, j, q = np.cos(half), v[..., 0] * k, v[..., 1] * k, v[..., 2] * k
    two_s = 2.0 / (r * r + i * i + j * j + q * q)
    r00 = 1.0 - two_s * (j * j + q * q)
    r01 = two_s * (i * j - q * r)
    r02 = two_s * (i * q + j * r)
    r12 = two_s * (j * q - i * r)
    r22 = 1.0 - two_s * (i * i + j * j)
    return np.degrees(np.stack([np.arctan2(-r12, r22), np.arcsin(np.clip(r02, -1.0, 1.0)), np.arctan2(-r01, r00)], -1))


def euler_deg_to_matrix(deg: np.ndarray) -> np.ndarray:
    """[..., 3] Euler 'XYZ' degrees -> [..., 3, 3] = Rx(X) Ry(Y) Rz(Z), float64."""
    a, b, c = np.moveaxis(np.radians(np.asarray(deg, dtype=np.float64)), -1, 0)
    sa, ca, sb, cb, sc, cc = np.sin(a), np.cos(a), np.sin(b), np.cos(b), np.sin(c), np.cos(c)
    rows = [cb * cc, -cb * sc, sb,
            sa * sb * cc + ca * sc, ca * cc - sa * sb * sc, -sa * cb,
            sa * sc - ca * sb * cc, ca * sb * sc + sa * cc, ca * cb]
    return np.stack(rows, -1).reshape(a.shape + (3, 3))


def axis_angle_to_matrix(v: np.ndarray) -> np.ndarray:
    """Rodrigues: R = I + sin(t) K + (1 - cos t) K^2 with K the cross-product matrix of the unit axis, float64."""
    v = np.asarray(v, dtype=np.float64)
    t = np.sqrt((v * v).sum(-1))
    u = v / np.where(t > 0, t, 1.0)[..., None]
    K = np.zeros(v.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -u[..., 2], u[..., 1], u[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -u[..., 0], -u[..., 1], u[..., 0]
    s, c1 = np.sin(t)[..., None, None], (1.0 - np.cos(t))[..., None, None]
    return np.eye(3) + s * K + c1 * (K @ K)


def matrix_quaternion_parts(m: np.ndarray) -> np.ndarray:
    """The four |q| components [..., 4] the candidate choice looks at."""
    d0, d1, d2 = m[..., 0, 0], m[..., 1, 1], m[..., 2, 2]
    t = np.stack([1 + d0 + d1 + d2, 1 + d0 - d1 - d2, 1 - d0 + d1 - d2, 1 - d0 - d1 + d2], -1)
    return np.sqrt(np.maximum(t, 0.0))


def euler_deg_to_axis_angle(deg: np.ndarray) -> np.ndarray:
    """[..., 3] Euler 'XYZ' degrees -> [..., 3] axis-angle vectors (rad), float64, by the reference's route."""
    m = euler_deg_to_matrix(deg)
    qa = matrix_quaternion_parts(m)
    best = qa.argmax(-1)
    m01, m02, m10, m12, m20, m21 = m[..., 0, 1], m[..., 0, 2], m[..., 1, 0], m[..., 1, 2], m[..., 2, 0], m[..., 2, 1]
    cand = np.stack([np.stack([qa[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], -1),
                     np.stack([m21 - m12, qa[..., 1] ** 2, m10 + m01, m02 + m20], -1),
                     np.stack([m02 - m20, m10 + m01, qa[..., 2] ** 2, m12 + m21], -1),
                     np.stack([m10 - m01, m20 + m02, m21 + m12, qa[..., 3] ** 2], -1)], -2)
    cand = cand / (2.0 * np.maximum(qa, 0.1))[..., None]
    q = np.take_along_axis(cand, best[..., None, None], -2)[..., 0, :]
    norm = np.sqrt((q[..., 1:] ** 2).sum(-1))
    half = np.arctan2(norm, q[..., 0])
    angle = 2.0 * half
    return q[..., 1:] / _sin_half_over_angle(half, angle)[..., None]


def joints(x: np.ndarray) -> np.ndarray:
    """[..., 3 J] -> [..., J, 3]"""
    x = np.asarray(x)
    return x.reshape(x.shape[:-1] + (x.shape[-1] // 3, 3))


def wrap360(d: np.ndarray) -> np.ndarray:
    """Angle differences in degrees modulo 360, in [-180, 180)."""
    return (np.asarray(d, dtype=np.float64) + 180.0) % 360.0 - 180.0


def forward_chain(x_std, stats) -> np.ndarray:
    """Standardised axis-angle [..., 3 J] -> Euler degrees [..., 3 J], float64 (statistics: dict of [3 J] arrays)."""
    v = np.asarray(x_std, np.float64) * np.asarray(stats["std_axis_angle"], np.float64) + np.asarray(stats["mean_axis_angle"], np.float64)
    return axis_angle_to_euler_deg(joints(v)).reshape(v.shape)


def inverse_chain(x_std, stats) -> np.ndarray:
    """Standardised Euler [..., 3 J] -> axis-angle vectors (rad) [..., 3 J], float64."""
    d = np.asarray(x_std, np.float64) * np.asarray(stats["std_euler"], np.float64) + np.asarray(stats["mean_euler"], np.float64)
    return euler_deg_to_axis_angle(joints(d)).reshape(d.shape)


def well_conditioned(euler_deg_f64: np.ndarray) -> np.ndarray:
    """Per joint [..., J]: |cos Y| > 0.1, where the three angles are well determined."""
    return np.abs(np.cos(np.radians(joints(euler_deg_f64)[..., 1]))) > 0.1


def settled(euler_deg_in_f64: np.ndarray, aa_f64: np.ndarray) -> np.ndarray:
    """Per joint [..., J]: the two largest |q| components are more than 1e-3 apart and the angle is more than 0.05 from pi - away from
    both, the candidate choice and the theta / theta - 2 pi form of the vector cannot flip under rounding."""
    qa = np.sort(matrix_quaternion_parts(euler_deg_to_matrix(joints(euler_deg_in_f64))), -1)
    ang = np.sqrt((joints(aa_f64) ** 2).sum(-1))
    return (qa[..., 3] - qa[..., 2] > 1e-3) & (np.abs(ang - np.pi) > 0.05)
