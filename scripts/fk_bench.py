#!/usr/bin/env python3
"""What joint positions cost, at the 9 000-frame stream [1, 9000, 192] and a 256 x 34 batch, on a seeded random skeleton
of BEAT's sizes (90 joints, 47 driven):

  (a) the device pass: glue.joint_positions on the sampler's [B, T, 192] result (gesture columns read in place), result left on the device;
  (b) its vector-Jacobian product (dsh_fk_positions_vjp) for a given dL/dpos;
  (c) the tail a user has without them: device-to-host copy, the same walk with torch in fp32 on 16 CPU threads (vectorised over the rows,
      a Python loop over the joints), positions left on the host.

Medians of five, the three alternated in one process.  A single launch of a few tens of microseconds cannot be timed between two events
from Python: the host needs longer than that to get from one record to the next.  So (a) and (b) are timed as BATCH back-to-back calls of
the prepared call object (output allocation + the C call, nothing else) between two events, divided by BATCH; the time of ONE call of the
public entry glue.joint_positions (argument checks, allocation, launch; host-bound) is reported beside it as entry_s.  Also reported: the
largest difference of (a) and (c) relative to the bone length (a sanity figure, not a gate).  Prints one JSON line per size; --out also writes them to a file.

Usage:  python scripts/fk_bench.py [--rounds 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffsheg_amd import glue  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.synthetic import make_pose_stat_vectors  # noqa: E402

BATCH = 50
SIZES = {"stream_9000": (1, 9000), "batch_256x34": (256, 34)}


def random_skeleton(J: int, Jc: int, seed: int) -> glue.Skeleton:
    rng = np.random.RandomState(seed)
    parents = [-1] + [int(rng.randint(max(0, j - 8), j)) for j in range(1, J)]
    return glue.Skeleton(parents, rng.uniform(-10, 10, size=(J, 3)).astype(np.float32), rng.permutation(J)[:Jc],
                         rest=rng.uniform(-180, 180, size=(J, 3)))


def host_positions(x: torch.Tensor, sk: glue.Skeleton, st: dict) -> torch.Tensor:
    """The walk with torch on the host, fp32: [rows, C] -> [rows, J, 3]."""
    n = 3 * sk.channels
    v = (x[:, :n] * st["std_axis_angle"] + st["mean_axis_angle"]).reshape(-1, sk.channels, 3)
    angle = v.norm(dim=-1)
    half = 0.5 * angle
    small = angle < 1e-6
    k = torch.where(small, 0.5 - angle * angle / 48, torch.sin(half) / torch.where(small, torch.ones_like(angle), angle))
    r, (i, j, q) = torch.cos(half), (v * k[..., None]).unbind(-1)
    s = 2.0 / (r * r + i * i + j * j + q * q)
    R = torch.stack([1 - s * (j * j + q * q), s * (i * j - q * r), s * (i * q + j * r), s * (i * j + q * r), 1 - s * (i * i + q * q),
                     s * (j * q - i * r), s * (i * q - j * r), s * (j * q + i * r), 1 - s * (i * i + j * j)], -1).reshape(-1, sk.channels, 3, 3)
    rest, off = torch.from_numpy(sk.rest_rot.astype(np.float32)), torch.from_numpy(sk.offsets.astype(np.float32))
    W, P = [], []
    for jt in range(sk.joints):
        c = int(sk.joint_channel[jt])
        Rj = R[:, c] if c >= 0 else rest[jt].expand(x.shape[0], 3, 3)
        if jt == 0:
            W.append(Rj)
            P.append(off[0].expand(x.shape[0], 3))
        else:
            p = int(sk.parents[jt])
            W.append(W[p] @ Rj)
            P.append(P[p] + W[p] @ off[jt])
    return torch.stack(P, 1)


def run(name: str, rounds: int) -> dict:
    cfg = get_config("beat")
    B, T = SIZES[name]
    dev = "cuda:0"
    sk = random_skeleton(90, cfg.split_pos // 3, 2024)
    st = make_pose_stat_vectors(sk.channels, 7102)
    stats = glue.PoseStats(**st, device=dev)
    x = torch.randn(B, T, cfg.net_dim_pose, generator=torch.Generator().manual_seed(1)).to(dev)
    g = torch.randn(B, T, sk.joints, 3, generator=torch.Generator().manual_seed(2)).to(dev)
    call = glue._FkCall(x, sk, stats.mean_axis_angle, stats.std_axis_angle, 0, None, 0, False)
    for _ in range(3):
        pos = glue.joint_positions(x, sk, stats, split_pos=cfg.split_pos)
        call.vjp(x, g)
    host_positions(x.cpu().reshape(B * T, -1), sk, st)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_fwd, t_vjp, t_entry, t_d2h, t_cpu = [], [], [], [], []
    for _ in range(rounds):
        for fn, sink, n in ((lambda: call.forward(x), t_fwd, BATCH), (lambda: call.vjp(x, g), t_vjp, BATCH),
                            (lambda: glue.joint_positions(x, sk, stats, split_pos=cfg.split_pos), t_entry, 1)):
            torch.cuda.synchronize()
            ev[0].record()
            for _i in range(n):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            sink.append(ev[0].elapsed_time(ev[1]) * 1e-3 / n)
        t0 = time.perf_counter()
        xh = x.cpu()
        t1 = time.perf_counter()
        ph = host_positions(xh.reshape(B * T, -1), sk, st)
        t2 = time.perf_counter()
        t_d2h.append(t1 - t0), t_cpu.append(t2 - t1)
    med = lambda v: float(np.median(v))                  # noqa: E731
    diff = float((pos.cpu().reshape(B * T, sk.joints, 3) - ph).abs().max()) / sk.bone_length
    host = {"d2h_s": med(t_d2h), "torch_cpu_s": med(t_cpu)}
    host["total_s"] = sum(host.values())
    return {"size": name, "batch": B, "frames": T, "joints": sk.joints, "driven": sk.channels, "rounds": rounds, "calls_per_timing": BATCH,
            "forward_s": med(t_fwd), "vjp_s": med(t_vjp), "entry_s": med(t_entry), "host_tail": host, "host_threads": torch.get_num_threads(),
            "speedup_forward": host["total_s"] / med(t_fwd), "speedup_entry": host["total_s"] / med(t_entry),
            "max_position_diff_over_bone_length": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lines = []
    for name in SIZES:
        lines.append(json.dumps(run(name, args.rounds)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
