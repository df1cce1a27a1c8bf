#!/usr/bin/env python3
"""What one validation step costs behind the sampler, for the SHOW 950-clip and BEAT 256-clip batches:

  (a) the sampling step as bench.py times it (generate_batch, bf16, ddim25, fresh conditioning every step);
  (b) the device tail: two FGD encodes + MSE / PCK / diversity, results left on the device;
  (c) the tail a user has without (b): device-to-host copy of both tensors, then the reference's host computation restated with
      torch / numpy on 16 threads (the FGD encoder as tests/metrics_ref.py states it, the diversity double loop in numpy).

There is no parent-commit time for (b): (c) is the baseline.  Also checked: (b) enqueues without any host synchronisation (the host time
to enqueue it is reported next to its device time; a hidden sync would make the two equal) and the samples of a step are bit-identical
with and without the tail.  Prints one JSON line per dataset; --out also writes them to a file.

Usage:  python scripts/validation_bench.py [--datasets show,beat] [--steps 3] [--host-clips 64] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from diffsheg_amd import metrics  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.model import UniDiffuser  # noqa: E402
from diffsheg_amd.synthetic import make_inputs, make_motion_pair  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from diffsheg_amd.weights import FID_VAE_LENGTH, make_synthetic_fid_state_dict, make_synthetic_state_dict  # noqa: E402
from metrics_ref import encode_ref  # noqa: E402

BATCH = {"show": 950, "beat": 256}


def host_tail(sd_fid, cfg, outputs: torch.Tensor, motions: torch.Tensor, joint_dim: int, host_clips: int) -> dict:
    """(c) on the host.  The encoder is timed on `host_clips` clips per side and scaled to the batch (it is linear in the batch); the
    metric lines and the diversity double loop run on the whole batch."""
    t0 = time.perf_counter()
    o, m = outputs.cpu(), motions.cpu()
    t_copy = time.perf_counter() - t0
    n = min(host_clips, o.shape[0])
    t0 = time.perf_counter()
    with torch.no_grad():
        encode_ref(sd_fid, o[:n], cfg.n_poses, FID_VAE_LENGTH)
        encode_ref(sd_fid, m[:n], cfg.n_poses, FID_VAE_LENGTH)
    t_enc = (time.perf_counter() - t0) * o.shape[0] / n
    B, T, C = o.shape
    on = o.numpy().reshape(B, T, C // joint_dim, joint_dim)
    mn = m.numpy().reshape(B, T, C // joint_dim, joint_dim)
    t0 = time.perf_counter()
    sq = (on - mn) ** 2
    float(np.mean(np.sqrt(np.sum(sq, axis=3)) < 0.5)), float(np.mean(sq))
    t_mp = time.perf_counter() - t0
    b_div = min(50, B)
    t0 = time.perf_counter()
    for g in range(B // b_div):
        grp, acc = on[g * b_div:(g + 1) * b_div], 0.0
        for i in range(b_div):
            for j in range(i + 1, b_div):
                acc += np.mean(np.absolute(grp[i] - grp[j]))
    t_div = time.perf_counter() - t0
    return {"d2h_s": t_copy, "encoder_s": t_enc, "encoder_clips_timed": 2 * n, "mse_pck_s": t_mp, "diversity_s": t_div,
            "total_s": t_copy + t_enc + t_mp + t_div}


def run(ds: str, steps: int, host_clips: int) -> dict:
    cfg = get_config(ds)
    B, jd = BATCH[ds], (1 if ds == "show" else 3)
    dev = "cuda:0"
    model = UniDiffuser(cfg, make_synthetic_state_dict(cfg, 1234), device=dev, precision="bf16")
    sd_fid = make_synthetic_fid_state_dict(cfg, 4321)
    net = metrics.HalfEmbeddingNet(cfg, sd_fid, device=dev)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    small = make_inputs(cfg, 64, seed=3)
    rep = (B + 63) // 64
    audio = small["audio_emb"].repeat(rep, 1, 1)[:B].to(dev).contiguous()
    hubert = small["pretrain_aud_feat"].repeat(rep, 1, 1)[:B].to(dev).contiguous()
    audio += 0.01 * torch.randn(audio.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    pid = torch.zeros(B, cfg.style_dim, device=dev)
    pid[torch.arange(B), torch.arange(B) % cfg.style_dim] = 1.0
    _, motions = make_motion_pair(cfg, B, 5)
    motions = motions.to(dev)

    def sample(i):
        model._cond_key = None
        return tr.generate_batch(audio, pid, cfg.net_dim_pose, {"pretrain_aud_feat": hubert}, {}, seed=2024 + i)

    def tail(outputs):
        r = metrics.batch_metrics(outputs, motions, jd)
        return r, net(outputs), net(motions)

    out = sample(-1)
    tail(out)                                            # warm-up: buffers, kernel attributes
    torch.cuda.synchronize()
    t_sample, t_tail, t_enq = [], [], []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for i in range(steps):
        ev[0].record()
        out = sample(i)
        ev[1].record()
        h0 = time.perf_counter()
        res = tail(out)
        t_enq.append(time.perf_counter() - h0)
        ev[2].record()
        torch.cuda.synchronize()
        t_sample.append(ev[0].elapsed_time(ev[1]) * 1e-3)
        t_tail.append(ev[1].elapsed_time(ev[2]) * 1e-3)
    again = sample(steps - 1)                            # the same step without the tail behind it
    torch.cuda.synchronize()
    host = host_tail(sd_fid, cfg, out, motions, jd, host_clips)
    fgd = metrics.frechet_distance(res[1].cpu().numpy(), res[2].cpu().numpy())
    med = lambda v: float(np.median(v))                  # noqa: E731
    return {"dataset": ds, "batch": B, "steps": steps, "sampling_step_s": med(t_sample), "device_tail_s": med(t_tail),
            "device_tail_enqueue_s": med(t_enq), "host_tail": host, "host_threads": torch.get_num_threads(),
            "samples_bit_identical_with_tail": bool(torch.equal(out, again)),
            "mse": float(res[0]["mse"]), "pck": float(res[0]["pck"]), "diversity_mean": float(res[0]["diversity"].mean()), "fgd": fgd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", default="show,beat")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--host-clips", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lines = []
    for ds in args.datasets.split(","):
        lines.append(json.dumps(run(ds, args.steps, args.host_clips)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
