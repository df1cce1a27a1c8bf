#!/usr/bin/env python3
"""Generate tests/golden/metrics_{show,beat}.npz: the validation metrics of the *imported reference* on seeded inputs.  Runs only in
the development container (the reference and scipy are needed here, never at test time).

Per dataset:
  * ``diffsheg_amd.weights.make_synthetic_fid_state_dict`` is loaded into the reference's own ``HalfEmbeddingNet`` with
    ``strict=True``, ``.eval()``; the latents of N_LATENT seeded clips of each of the two related inputs of
    ``diffsheg_amd.synthetic.make_motion_pair`` are stored, with the reference's ``calculate_frechet_distance``
    (utils/metrics.py, on its ``calculate_activation_statistics``) of the two latent sets.
  * MSE / PCK / diversity for B = 120 (two complete groups of 50, a dropped remainder of 20) and B = 7 (< 50).  These lines are inline
    in the reference's ``train()`` (trainers/ddpm_show_trainer.py:516-550, ddpm_beat_trainer.py:587-597) and none of its text may be
    copied, so they are NOT executed from the reference: the expected values are restated below from the issue's definitions, with
    numpy in float32 in the reference's order of operations (what makes the PCK count exact: per-element products, numpy's
    left-to-right sum over the joint axis of 3, a correctly rounded sqrt; the diversity pair means added sequentially in float32),
    and cross-checked against a float64 evaluation.  The script asserts that no joint lies within 1e-6 of the PCK threshold, where
    the order of three fp32 additions could decide (pick another seed if one does).

Inputs are never stored: both sides regenerate them from the seeds in the fixture.

Usage:  python tests/golden/make_golden_metrics.py --reference /path/to/DiffSHEG     (or DIFFSHEG_REFERENCE in the environment)
"""
from __future__ import annotations

import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.synthetic import make_motion_pair  # noqa: E402
from diffsheg_amd.weights import FID_VAE_LENGTH, make_synthetic_fid_state_dict  # noqa: E402

FID_SEED = 4321
N_LATENT = 64
LATENT_SEED = {"show": 11, "beat": 12}
METRIC_CASES = {"show": ((120, 2100), (7, 2200)), "beat": ((120, 3100), (7, 3200))}   # (batch, first seed tried)
JOINT_DIM = {"show": 1, "beat": 3}


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def import_reference(ref: str):
    sys.dont_write_bytecode = True
    if ref not in sys.path:
        sys.path.insert(0, ref)
    _stub("cv2", norm=None)                      # dead import at models/transformer.py:5 (models/__init__.py pulls it in)
    from models.motion_autoencoder import HalfEmbeddingNet
    from utils.metrics import calculate_activation_statistics, calculate_frechet_distance
    return HalfEmbeddingNet, calculate_activation_statistics, calculate_frechet_distance


def pck_margin(outputs: np.ndarray, motions: np.ndarray, joint_dim: int) -> float:
    """Smallest distance of a joint's error norm (float64) from the PCK threshold 0.5."""
    d64 = (outputs.astype(np.float64) - motions.astype(np.float64)).reshape(-1, joint_dim)
    return float(np.abs(np.sqrt(np.sum(d64 ** 2, axis=1)) - 0.5).min())


def expected_batch_metrics(outputs: np.ndarray, motions: np.ndarray, joint_dim: int) -> dict:
    B, T, C = outputs.shape
    o = outputs.reshape(B, T, C // joint_dim, joint_dim)
    m = motions.reshape(B, T, C // joint_dim, joint_dim)
    diff = o - m                                                    # float32
    sq = diff ** 2
    root = np.sqrt(np.sum(sq, axis=3))
    count = int(np.count_nonzero(root < 0.5))
    d64 = o.astype(np.float64) - m.astype(np.float64)
    root64 = np.sqrt(np.sum(d64 ** 2, axis=3))
    assert float(np.abs(root64 - 0.5).min()) >= 1e-6, "a joint lies within 1e-6 of the PCK threshold: pick another seed"
    assert count == int(np.count_nonzero(root64 < 0.5))
    mse = np.mean(sq)                                               # numpy's pairwise float32 mean, as the reference
    b_div = min(50, B)
    divs = []
    for g in range(B // b_div):
        grp = o[g * b_div:(g + 1) * b_div]
        acc = 0.0
        for i in range(b_div):
            for j in range(i + 1, b_div):
                acc += np.mean(np.absolute(grp[i] - grp[j]))        # 0.0 + np.float32 stays float32 (NumPy 2)
        divs.append(float(acc * 2 / (b_div * (b_div - 1))))
        g64 = grp.astype(np.float64).reshape(b_div, -1)
        ref64 = sum(np.abs(g64[i] - g64[i + 1:]).mean(axis=1).sum() for i in range(b_div - 1)) * 2 / (b_div * (b_div - 1))
        assert abs(divs[-1] - ref64) <= 1e-4 * ref64, (divs[-1], ref64)
    assert abs(float(mse) - float(np.mean(d64 ** 2))) <= 1e-5 * float(mse)
    return {"mse": float(mse), "mse_f64": float(np.mean(d64 ** 2)), "pck_count": count, "pck_total": int(root.size),
            "diversity": np.asarray(divs, dtype=np.float64), "b_div": b_div}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("DIFFSHEG_REFERENCE"), help="checkout of the reference implementation")
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(args.reference):
        ap.error("--reference (or DIFFSHEG_REFERENCE) must name a checkout of the reference implementation")
    HalfEmbeddingNet, act_stats, frechet = import_reference(args.reference)
    for ds in ("show", "beat"):
        cfg = get_config(ds)
        opt = argparse.Namespace(n_poses=cfg.n_poses, net_dim_pose=cfg.net_dim_pose, vae_length=FID_VAE_LENGTH)
        net = HalfEmbeddingNet(opt)
        net.load_state_dict(make_synthetic_fid_state_dict(cfg, FID_SEED), strict=True)
        net.eval()
        y, x = make_motion_pair(cfg, N_LATENT, LATENT_SEED[ds])
        with torch.no_grad():
            lat_x = net(x[:, :cfg.n_poses]).numpy()
            lat_y = net(y[:, :cfg.n_poses]).numpy()
        fgd = float(frechet(*act_stats(lat_y), *act_stats(lat_x)))
        out = {"fid_seed": FID_SEED, "latent_seed": LATENT_SEED[ds], "n_latent": N_LATENT, "latents_motions": lat_x,
               "latents_outputs": lat_y, "fgd": fgd, "joint_dim": JOINT_DIM[ds]}
        print(f"{ds}: latents |z| mean {np.abs(lat_x).mean():.3f}, range {lat_x.max() - lat_x.min():.3f}, FGD {fgd:.6f}")
        assert fgd >= 0.1, "the fixture's FGD has to be large enough for a relative gate"
        for k, (B, seed0) in enumerate(METRIC_CASES[ds]):
            # first seed from seed0 upwards with no joint within 1e-6 of the threshold (2.4 M entries with a density of ~0.8 per unit
            # around 0.5 leave ~4 such entries per SHOW batch on average: a clean seed is one in ~50)
            for seed in range(seed0, seed0 + 2000):
                o, m = make_motion_pair(cfg, B, seed)
                if pck_margin(o.numpy(), m.numpy(), JOINT_DIM[ds]) >= 1e-6:
                    break
            else:
                raise AssertionError("no seed with a clean PCK margin found")
            e = expected_batch_metrics(o.numpy(), m.numpy(), JOINT_DIM[ds])
            print(f"  B={B}: mse {e['mse']:.6f} pck {e['pck_count']}/{e['pck_total']} diversity {e['diversity']}")
            assert 0 < e["pck_count"] < e["pck_total"]
            out[f"case{k}_batch"], out[f"case{k}_seed"] = B, seed
            for name, v in e.items():
                out[f"case{k}_{name}"] = v
        path = os.path.join(HERE, f"metrics_{ds}.npz")
        np.savez(path, **out)
        print("  wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
