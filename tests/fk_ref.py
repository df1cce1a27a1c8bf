"""Torch emulation of the forward-kinematics semantics (include/diffsheg_hip.h, dsh_fk_positions / dsh_fk_positions_vjp), parameterised by
dtype and written from the mathematics; used only by tests.  Every operation is an elementwise torch op in the order the header states
(every 3-term product is (a0 b0 + a1 b1) + a2 b2), so the float32 run is the "reference's own float32 run" the GPU gates are derived
from, the float64 run is the truth, and autograd through either gives the gradient the VJP kernel is held to.

    v_i = x * std + mean  ->  R_j = exp([v_i]x) through the normalised quaternion (sin(t/2)/t, 1/2 - t^2/48 below 1e-6)
                              | kind "euler": deg -> rad -> Rx Ry Rz       | rest_rot[j] where no channel drives joint j
    W_0 = R_0, p_0 = offsets[0];   W_j = W_parent R_j,  p_j = p_parent + W_parent offsets[j]

A skeleton is a dict of numpy arrays: parents [J], offsets [J, 3], channel_joint [Jc], rest_rot [J, 3, 3] (offsets are values a
float32 holds; rest_rot is float64 and is rounded by the float32 run as the upload to the device rounds it).  ``mutant`` switches in one deliberate mistake, for the tests that show the gates reject it.

Also here: the skeletons, statistics and inputs of the GPU tests (tests/test_gpu_fk.py), so that the CPU tests can judge the mutants on
exactly those inputs."""
from __future__ import annotations

import numpy as np
import torch

SMALL = 1e-6        # quaternion series threshold
SMALL_JR = 1e-3     # right-Jacobian series threshold
MARGIN = 4.0        # every GPU gate is MARGIN x the float32 emulation's own error

FORWARD_MUTANTS = ("offset_by_own_rotation", "rotation_order", "rest_ignored")
VJP_MUTANTS = ("left_jacobian", "std_dropped")


# ---- the emulation -----------------------------------------------------------------------------------------------------------------------
def _t(a, dtype):
    return a.to(dtype) if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a)).to(dtype)


def aa_matrices(v: torch.Tensor) -> torch.Tensor:
    """[..., 3] axis-angle vectors -> [..., 3, 3], in v's dtype."""
    vx, vy, vz = v[..., 0], v[..., 1], v[..., 2]
    angle = torch.sqrt((vx * vx + vy * vy) + vz * vz)
    half = angle * 0.5
    small = angle.abs() < SMALL
    k = torch.where(small, 0.5 - (angle * angle) / 48.0, torch.sin(half) / torch.where(small, torch.ones_like(angle), angle))
    r, i, j, q = torch.cos(half), vx * k, vy * k, vz * k
    two_s = 2.0 / (((r * r + i * i) + j * j) + q * q)
    m = [1.0 - two_s * (j * j + q * q), two_s * (i * j - q * r), two_s * (i * q + j * r),
         two_s * (i * j + q * r), 1.0 - two_s * (i * i + q * q), two_s * (j * q - i * r),
         two_s * (i * q - j * r), two_s * (j * q + i * r), 1.0 - two_s * (i * i + j * j)]
    return torch.stack(m, -1).reshape(v.shape[:-1] + (3, 3))


def euler_matrices(deg: torch.Tensor) -> torch.Tensor:
    """[..., 3] Euler 'XYZ' degrees -> (Rx Ry) Rz, in deg's dtype; the degree -> radian step is deg * pi / 180 with pi in that dtype."""
    pi = torch.tensor(np.pi, dtype=deg.dtype)
    rad = deg * pi / 180.0
    a, b, c = rad[..., 0], rad[..., 1], rad[..., 2]
    sa, ca, sb, cb, sc, cc = torch.sin(a), torch.cos(a), torch.sin(b), torch.cos(b), torch.sin(c), torch.cos(c)
    a10, a20 = sa * sb, -(ca * sb)
    m = [cb * cc, -(cb * sc), sb,
         a10 * cc + ca * sc, ca * cc - a10 * sc, -(sa * cb),
         a20 * cc + sa * sc, sa * cc - a20 * sc, ca * cb]
    return torch.stack(m, -1).reshape(deg.shape[:-1] + (3, 3))


def _matmul(A, B):          # [..., 3, 3] x [..., 3, 3], (a0 b0 + a1 b1) + a2 b2
    return (A[..., :, 0:1] * B[..., 0:1, :] + A[..., :, 1:2] * B[..., 1:2, :]) + A[..., :, 2:3] * B[..., 2:3, :]


def _matvec(A, o):          # [..., 3, 3] x [3]
    return (A[..., :, 0] * o[0] + A[..., :, 1] * o[1]) + A[..., :, 2] * o[2]


def joint_channel(sk) -> np.ndarray:
    jc = np.full(len(sk["parents"]), -1, dtype=np.int64)
    jc[np.asarray(sk["channel_joint"])] = np.arange(len(sk["channel_joint"]))
    return jc


def denormalise(x, sk, mean, std, dtype):
    """x [rows, >= 3 Jc] -> v [rows, Jc, 3] in dtype"""
    n = 3 * len(sk["channel_joint"])
    v = _t(x, dtype)[:, :n] * _t(std, dtype) + _t(mean, dtype)
    return v.reshape(v.shape[0], n // 3, 3)


def forward(x, sk, mean, std, dtype=torch.float64, kind="axis_angle", mutant=None):
    """Positions [rows, J, 3] and world rotations [rows, J, 3, 3] of x [rows, >= 3 Jc] (a tensor that requires grad stays attached)."""
    v = denormalise(x, sk, mean, std, dtype)
    R_driven = aa_matrices(v) if kind == "axis_angle" else euler_matrices(v)
    rows, J = v.shape[0], len(sk["parents"])
    jc, off, rest = joint_channel(sk), _t(sk["offsets"], dtype), _t(sk["rest_rot"], dtype)
    if mutant == "rest_ignored":
        rest = torch.eye(3, dtype=dtype).expand(J, 3, 3)
    W, P = [], []
    for j in range(J):
        R = R_driven[:, jc[j]] if jc[j] >= 0 else rest[j].expand(rows, 3, 3)
        if j == 0:
            W.append(R)
            P.append(off[0].expand(rows, 3))
            continue
        p = int(sk["parents"][j])
        Wj = _matmul(R, W[p]) if mutant == "rotation_order" else _matmul(W[p], R)
        P.append(P[p] + _matvec(Wj if mutant == "offset_by_own_rotation" else W[p], off[j]))
        W.append(Wj)
    return torch.stack(P, 1), torch.stack(W, 1)


def _cross(a, b):
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def vjp(x, g, sk, mean, std, dtype=torch.float64, mutant=None):
    """dL/dx [rows, 3 Jc] for g = dL/dpos [rows, J, 3], by the header's recursion (no autograd)."""
    with torch.no_grad():
        P, W = forward(x, sk, mean, std, dtype)
        v = denormalise(x, sk, mean, std, dtype)
        J = len(sk["parents"])
        F = [_t(g, dtype)[:, j] for j in range(J)]
        M = [torch.zeros_like(F[0]) for _ in range(J)]
        for j in range(J - 1, 0, -1):
            p = int(sk["parents"][j])
            M[p] = M[p] + (M[j] + _cross(P[:, j] - P[:, p], F[j]))
            F[p] = F[p] + F[j]
        cj = np.asarray(sk["channel_joint"])
        Wd, Md = W[:, cj], torch.stack(M, 1)[:, cj]                         # [rows, Jc, 3, 3], [rows, Jc, 3]
        u = (Wd[..., 0, :] * Md[..., 0:1] + Wd[..., 1, :] * Md[..., 1:2]) + Wd[..., 2, :] * Md[..., 2:3]      # W^T M
        t = torch.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        small = t < SMALL_JR
        ts = torch.where(small, torch.ones_like(t), t)
        h = ts * 0.5
        sh = torch.sin(h) / h
        a = torch.where(small, 0.5 - (t * t) / 24.0, 0.5 * (sh * sh))
        b = torch.where(small, 1.0 / 6.0 - (t * t) / 120.0, (ts - torch.sin(ts)) / ((ts * ts) * ts))
        if mutant == "left_jacobian":
            a = -a
        c1 = _cross(v, u)
        c2 = _cross(v, c1)
        d = (u + a[..., None] * c1) + b[..., None] * c2
        if mutant != "std_dropped":
            d = _t(std, dtype).reshape(1, -1, 3) * d
        return d.reshape(d.shape[0], -1)


def autograd_vjp(x, g, sk, mean, std, dtype):
    """dL/dx [rows, 3 Jc] by torch autograd through forward() in dtype."""
    n = 3 * len(sk["channel_joint"])
    xx = _t(x, dtype)[:, :n].clone().requires_grad_(True)
    P, _ = forward(xx, sk, mean, std, dtype)
    if not P.requires_grad:                 # a single root: the positions do not depend on x at all
        return torch.zeros_like(xx)
    (gx,) = torch.autograd.grad(P, xx, _t(g, dtype))
    return gx


# ---- skeletons -----------------------------------------------------------------------------------------------------------------------------
def euler_deg_to_matrix64(deg):
    return euler_matrices(torch.as_tensor(np.asarray(deg, dtype=np.float64))).numpy()


def _skeleton(parents, offsets, channel_joint, rest=None):
    """Offsets are values a float32 holds.  The rest rotations are folded in float64, as glue.Skeleton folds them, and stay float64 here:
    the truth runs on the exact rotations, and the float32 emulation rounds them exactly as the upload to the device does.  (A rounded
    rest rotation is orthogonal only to 1e-7, and W^T M in the VJP assumes orthogonal world rotations: with rounded matrices in the
    float64 run the recursion and autograd differ by 4e-8, measured - a rounding effect the float32 yardstick carries, not the truth.)"""
    J = len(parents)
    off = np.asarray(offsets, dtype=np.float32).astype(np.float64).reshape(J, 3)
    rest_deg = np.zeros((J, 3)) if rest is None else np.asarray(rest, dtype=np.float64)
    rest_rot = euler_deg_to_matrix64(rest_deg)
    return {"parents": np.asarray(parents, dtype=np.int64), "offsets": off, "channel_joint": np.asarray(channel_joint, dtype=np.int64),
            "rest_deg": rest_deg, "rest_rot": rest_rot, "bone_length": float(np.sqrt((off ** 2).sum(-1)).sum())}


def _random_tree(J, Jc, seed, reach):
    rng = np.random.RandomState(seed)
    parents = [-1] + [int(rng.randint(max(0, j - reach), j)) for j in range(1, J)]
    offsets = rng.uniform(-10.0, 10.0, size=(J, 3))
    cj = rng.permutation(J)[:Jc]
    rest = rng.uniform(-180.0, 180.0, size=(J, 3))
    return _skeleton(parents, offsets, cj, rest)


def skeleton(name):
    if name == "single":
        return _skeleton([-1], [[1.0, 2.0, 3.0]], [0])
    if name == "chain3":                    # the known-answer chain: unit bones along x
        return _skeleton([-1, 0, 1], [[0, 0, 0], [1, 0, 0], [1, 0, 0]], [0, 1, 2])
    if name == "tree7":                     # root 0; branch 1 - 2 - 3 (3 an end site); branch 4 - 5 - 6 with 5 undriven, at a rest rotation
        return _skeleton([-1, 0, 1, 2, 0, 4, 5],
                         [[0.5, 9.0, -1.0], [2.0, 1.0, 0.0], [3.0, 0.0, 0.5], [1.5, 0.0, 0.0], [-2.0, 1.0, 0.0], [-3.0, 0.5, 0.25], [-1.0, -2.0, 4.0]],
                         [4, 0, 2, 6, 1], rest=[[0, 0, 0]] * 5 + [[30.0, -50.0, 110.0], [0, 0, 0]])
    if name == "rand90":                    # BEAT's sizes: 47 driven joints of 90
        return _random_tree(90, 47, 2024, 8)
    if name == "big256":
        return _random_tree(256, 200, 2025, 4)
    raise KeyError(name)


SKELETONS = ("single", "chain3", "tree7", "rand90", "big256")
ROW_COUNTS = (1, 5, 257)


def statistics(Jc, seed):
    """mean / std of the input kind, float32 values [3 Jc]"""
    rng = np.random.RandomState(seed)
    return (rng.normal(0.0, 0.1, 3 * Jc).astype(np.float32), rng.uniform(0.5, 1.5, 3 * Jc).astype(np.float32))


def inputs(Jc, rows, seed, mean, std):
    """Standardised axis-angle rows [rows, 3 Jc] float32: |v| uniform in (0, pi], and in every row one joint at |v| = 5e-7 (below the
    quaternion's series threshold; not exactly 0, where the truth's autograd is undefined) and one at 2 pi - 0.05."""
    rng = np.random.RandomState(seed)
    d = rng.normal(size=(rows, Jc, 3))
    d /= np.sqrt((d * d).sum(-1, keepdims=True))
    mag = rng.uniform(1e-2, np.pi, size=(rows, Jc))
    r = np.arange(rows)
    if Jc > 1:
        mag[r, r % Jc] = 5e-7
        mag[r, (r + 1) % Jc] = 2 * np.pi - 0.05
    else:
        mag[r % 3 == 0, 0] = 5e-7
        mag[r % 3 == 1, 0] = 2 * np.pi - 0.05
    v = (d * mag[..., None]).reshape(rows, 3 * Jc)
    return ((v - mean.astype(np.float64)) / std.astype(np.float64)).astype(np.float32)


def cotangent(J, rows, seed):
    """g [rows, J, 3] float32: seeded random rows; rows 1 and 3 (when there) are zero except on the LAST joint, always a leaf."""
    g = np.random.RandomState(seed).normal(size=(rows, J, 3)).astype(np.float32)
    for r in (1, 3):
        if r < rows:
            g[r, :-1] = 0.0
    return g


def ancestors(sk, j):
    out = []
    while sk["parents"][j] >= 0:
        j = int(sk["parents"][j])
        out.append(j)
    return out


_CASES = {}


def case(name):
    """Everything the tests of one skeleton share, computed once and never modified: the skeleton, statistics, the 257 input rows and
    cotangents, the float64 truth, the float32 emulation and the yardsticks eps_ref (the float32 emulation's own error)."""
    if name not in _CASES:
        sk = skeleton(name)
        J, Jc = len(sk["parents"]), len(sk["channel_joint"])
        rows = max(ROW_COUNTS)
        mean, std = statistics(Jc, 11 + J)
        x = inputs(Jc, rows, 100 + J, mean, std)
        g = cotangent(J, rows, 200 + J)
        with torch.no_grad():
            p64, w64 = forward(x, sk, mean, std, torch.float64)
            p32, w32 = forward(x, sk, mean, std, torch.float32)
        g64 = autograd_vjp(x, g, sk, mean, std, torch.float64)
        g32 = autograd_vjp(x, g, sk, mean, std, torch.float32)
        gscale = max(float(g64.abs().max()), 1e-300)
        eps = {"pos": float((p32.double() - p64).abs().max()) / sk["bone_length"], "wrot": float((w32.double() - w64).abs().max()),
               "vjp": float((g32.double() - g64).abs().max()) / gscale}
        _CASES[name] = dict(sk=sk, J=J, Jc=Jc, mean=mean, std=std, x=x, g=g, pos64=p64, wrot64=w64, grad64=g64, gscale=gscale, eps=eps)
    return _CASES[name]


def forward_errors(pos, wrot, c):
    """(position error / bone length, rotation error as matrices) of a result against the case's float64 truth, over its first rows"""
    n = pos.shape[0]
    pos, wrot = torch.as_tensor(pos).double().reshape(n, c["J"], 3), torch.as_tensor(wrot).double().reshape(n, c["J"], 3, 3)
    return float((pos - c["pos64"][:n]).abs().max()) / c["sk"]["bone_length"], float((wrot - c["wrot64"][:n]).abs().max())


def vjp_error(grad, c):
    n = grad.shape[0]
    return float((torch.as_tensor(grad).double().reshape(n, -1) - c["grad64"][:n]).abs().max()) / c["gscale"]
