#!/usr/bin/env python3
"""Generate tests/golden/rotations_beat.npz: the BEAT Euler tail of the *imported reference* on seeded inputs.  Runs only in the
development container (the reference is needed here, never at test time).

The reference's ``datasets/rotation_converter.py`` is loaded by file path (its ``datasets`` package cannot be imported: the package's
``__init__`` needs lmdb) and run on the two chains exactly as the reference calls it:

  forward  (trainers/ddpm_beat_trainer.py:1056-1060)  x * std_aa + mean_aa -> axis_angle_to_euler_angles -> * (180 / pi)
                                                      -> (deg - mean_e) / std_e
  inverse  (datasets/beat.py:380-383, :401)           x * std_e + mean_e -> * pi / 180 -> euler_angles_to_axis_angle(., "XYZ")
                                                      -> (aa - mean_aa) / std_aa

each in float64 (the truth) and in float32 (the yardstick: its distance from the truth is the error a correct fp32 implementation has).
The fixture holds numeric arrays only - seeds, shapes, expected outputs, masks and flags; inputs and statistics are regenerated from the
seeds by ``diffsheg_amd.synthetic`` on both sides.

Random block: B = 2, T = 17, J = 47, standardised inputs ~ N(0, 1), synthetic statistics (``make_pose_stat_vectors``).
Edge block (``make_rotation_edge_cases``; statistics mean 0 / std 1, so the values land exactly): the zero vector, either side of the
small-angle threshold, angles around and beyond pi, six gimbal joints; for the inverse |Y| = 89.9 degrees and half turns (w ~ 0).
Masks (per joint, by the float64 results): ``well_conditioned`` = |cos Y| > 0.1 (angles comparable), ``settled`` = the two largest |q|
candidates more than 1e-3 apart and |angle - pi| > 0.05 (vectors comparable).  Edge flags: ``edge_fwd_gimbal`` (the six joints within
0.5 degrees of gimbal lock: matrices only), ``edge_fwd_exact_gimbal`` (two more, exactly on it: cos Y = 0 leaves X and Z undetermined
in every fp32 run, the reference's included - ``edge_exact_gimbal_ref_mat_err`` records how far its float32 run is from its float64 run
as a matrix there - so only Y is comparable), ``edge_fwd_zero`` (exact zeros in -> exact zeros out).  ``eps_*``: the reference's float32
error against its float64 run per block, quantity and group of joints (the tests recompute them from the arrays).  The script fails if
a mask leaves out more than 1 % of the random block.

Usage:  python tests/golden/make_golden_rotations.py --reference /path/to/DiffSHEG     (or DIFFSHEG_REFERENCE in the environment)
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import rotation_ref as rr  # noqa: E402
from diffsheg_amd.synthetic import make_pose_stat_vectors, make_rotation_edge_cases, make_rotation_inputs  # noqa: E402

B, T, J = 2, 17, 47
INPUT_SEED, STATS_SEED = 7101, 7102


def load_converter(ref: str):
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("reference_rotation_converter", os.path.join(ref, "datasets", "rotation_converter.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def forward(rc, x, st, dtype):
    x, (m_aa, s_aa, m_e, s_e) = x.to(dtype), (st[k].to(dtype) for k in ("mean_axis_angle", "std_axis_angle", "mean_euler", "std_euler"))
    denorm = x * s_aa + m_aa
    b, t, c = denorm.shape
    e = rc.axis_angle_to_euler_angles(denorm.reshape(b, t, c // 3, 3)).reshape(b, t, c)
    e = e * (180 / np.pi)
    return e.numpy(), ((e - m_e) / s_e).numpy()


def inverse(rc, x, st, dtype):
    x, (m_aa, s_aa, m_e, s_e) = x.to(dtype), (st[k].to(dtype) for k in ("mean_axis_angle", "std_axis_angle", "mean_euler", "std_euler"))
    d = x * s_e + m_e
    r = d * np.pi / 180.0
    b, t, c = r.shape
    aa = rc.euler_angles_to_axis_angle(r.reshape(b, t, c // 3, 3), "XYZ").reshape(b, t, c)
    return aa.numpy(), ((aa - m_aa) / s_aa).numpy()


def unit_stats(n):
    z, o = torch.zeros(n), torch.ones(n)
    return {"mean_axis_angle": z, "std_axis_angle": o, "mean_euler": z, "std_euler": o}


def mat_err(deg_a, deg_b):
    return np.abs(rr.euler_deg_to_matrix(rr.joints(deg_a)) - rr.euler_deg_to_matrix(rr.joints(deg_b))).max(axis=(-1, -2))


def aa_mat_err(aa_a, aa_b):
    return np.abs(rr.axis_angle_to_matrix(rr.joints(aa_a)) - rr.axis_angle_to_matrix(rr.joints(aa_b))).max(axis=(-1, -2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("DIFFSHEG_REFERENCE"), help="checkout of the reference implementation")
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(args.reference):
        ap.error("--reference (or DIFFSHEG_REFERENCE) must name a checkout of the reference implementation")
    rc = load_converter(args.reference)
    out = {"batch": B, "frames": T, "joints": J, "input_seed": INPUT_SEED, "stats_seed": STATS_SEED}

    # ---- random block ----
    st = make_pose_stat_vectors(J, STATS_SEED)
    x_aa, x_eu = make_rotation_inputs(B, T, J, INPUT_SEED)
    deg64, _ = forward(rc, x_aa, st, torch.float64)
    deg32, std32 = forward(rc, x_aa, st, torch.float32)
    aa64, _ = inverse(rc, x_eu, st, torch.float64)
    aa32, aastd32 = inverse(rc, x_eu, st, torch.float32)
    assert np.isfinite(deg64).all() and np.isfinite(aa64).all()
    wc = rr.well_conditioned(deg64)
    d_in64 = x_eu.double().numpy() * st["std_euler"].double().numpy() + st["mean_euler"].double().numpy()
    se = rr.settled(d_in64, aa64)
    out.update(euler_deg_f64=deg64, euler_deg_f32=deg32, euler_std_f32=std32, aa_f64=aa64, aa_f32=aa32, aa_std_f32=aastd32,
               well_conditioned=wc, settled=se)
    left_a, left_v = 1.0 - wc.mean(), 1.0 - se.mean()
    print(f"random block: {wc.size} joints, angle comparison leaves out {int((~wc).sum())} ({100 * left_a:.2f} %), "
          f"vector comparison {int((~se).sum())} ({100 * left_v:.2f} %)")
    assert left_a <= 0.01 and left_v <= 0.01, "a mask leaves out more than 1 % of the random block"
    eps = {"eps_fwd_deg": np.abs(rr.wrap360(rr.joints(deg32) - rr.joints(deg64)))[wc].max(),
           "eps_fwd_mat": np.nanmax(mat_err(deg32, deg64)),
           "eps_inv_vec": np.abs(rr.joints(aa32) - rr.joints(aa64))[se].max(),
           "eps_inv_mat": np.nanmax(aa_mat_err(aa32, aa64))}

    # ---- edge block ----
    edge = make_rotation_edge_cases()
    n_f, n_i = edge["axis_angle"].shape[-1], edge["euler"].shape[-1]
    e_deg64, _ = forward(rc, edge["axis_angle"], unit_stats(n_f), torch.float64)
    e_deg32, _ = forward(rc, edge["axis_angle"], unit_stats(n_f), torch.float32)
    e_aa64, _ = inverse(rc, edge["euler"], unit_stats(n_i), torch.float64)
    e_aa32, _ = inverse(rc, edge["euler"], unit_stats(n_i), torch.float32)
    assert np.isfinite(e_deg64).all() and np.isfinite(e_aa64).all(), "the float64 truth has to be finite on every edge joint"
    e_wc = rr.well_conditioned(e_deg64)
    gimbal, exact, zero = (np.zeros(n_f // 3, dtype=bool) for _ in range(3))
    gimbal[6:12], exact[12:14], zero[0] = True, True, True
    y = np.abs(rr.joints(e_deg64)[0, 0, :, 1])
    assert (np.abs(y[gimbal] - 90.0) <= 0.5).all() and (np.abs(y[gimbal] - 90.0) >= 0.04).all() and (np.abs(y[exact] - 90.0) < 1e-4).all()
    assert not e_wc[0, 0][gimbal | exact].any() and e_wc[0, 0][~(gimbal | exact)].all()
    e_se = rr.settled(edge["euler"].double().numpy(), e_aa64)
    out.update(edge_euler_deg_f64=e_deg64, edge_euler_deg_f32=e_deg32, edge_aa_f64=e_aa64, edge_aa_f32=e_aa32,
               edge_fwd_well_conditioned=e_wc, edge_fwd_gimbal=gimbal, edge_fwd_exact_gimbal=exact, edge_fwd_zero=zero,
               edge_inv_settled=e_se)
    print("edge forward: float32 run of the reference NaN at joints", np.nonzero(~np.isfinite(rr.joints(e_deg32)).all(-1)[0, 0])[0].tolist())
    print("edge forward |f32 - f64| deg per joint:", np.abs(rr.wrap360(rr.joints(e_deg32) - rr.joints(e_deg64))).max(-1)[0, 0])
    print("edge forward matrix err per joint:", mat_err(e_deg32, e_deg64)[0, 0])
    print("edge inverse settled:", e_se[0, 0].astype(int), " matrix err per joint:", aa_mat_err(e_aa32, e_aa64)[0, 0])
    eps.update(eps_edge_fwd_deg=np.abs(rr.wrap360(rr.joints(e_deg32) - rr.joints(e_deg64)))[e_wc].max(),
               eps_edge_fwd_mat=np.nanmax(mat_err(e_deg32, e_deg64)[0, 0][~(gimbal | exact)]),
               eps_edge_fwd_mat_gimbal=np.nanmax(mat_err(e_deg32, e_deg64)[0, 0][gimbal]),
               eps_edge_fwd_y_gimbal=np.nanmax(np.abs(rr.joints(e_deg32) - rr.joints(e_deg64))[0, 0, :, 1][gimbal | exact]),
               edge_exact_gimbal_ref_mat_err=np.nanmax(mat_err(e_deg32, e_deg64)[0, 0][exact]),
               eps_edge_inv_vec=np.abs(rr.joints(e_aa32) - rr.joints(e_aa64))[e_se].max(),
               eps_edge_inv_mat=np.nanmax(aa_mat_err(e_aa32, e_aa64)))
    for k, v in eps.items():
        print(f"  {k} = {float(v):.3e}")
        out[k] = float(v)
    path = os.path.join(HERE, "rotations_beat.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
