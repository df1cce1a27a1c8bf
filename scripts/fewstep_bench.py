#!/usr/bin/env python3
"""Few-step sampling on one MI355X (SHOW, bf16): time and distance per sampling configuration.

  python scripts/fewstep_bench.py [--batch 950] [--steps 3] [--warmup 1]

Configurations: (25, ddim, ddim) — today's default, the baseline of every ratio below, measured in the same run —, (10, ddim, ddim),
(10, logsnr, dpm2m), (8, logsnr, dpm2m), set with ``DDPMTrainer.set_sampling``.  For each one:

  * motion frames/s of the --batch clip batch, of one clip alone and of one chained (out-painting) window of one clip; the
    expectation is time proportional to the number of denoiser evaluations (printed beside it);
  * the distance of its result to a 'ddim250' result from the same seed (the same x_T), B = 2, on the synthetic weights:
    max |x - x250| / max |x250|.  Reported, not gated: random weights are not a smooth score field and |x| grows to ~1e3.

Prints one JSON line per configuration and a closing summary line.  bench.py stays the yardstick of the headline figure.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from diffsheg_amd import _lib  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.model import UniDiffuser  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from diffsheg_amd.weights import make_synthetic_state_dict  # noqa: E402

CONFIGS = [(25, "ddim", "ddim"), (10, "ddim", "ddim"), (10, "logsnr", "dpm2m"), (8, "logsnr", "dpm2m")]


def inputs(cfg, B, T, seed):
    small = make_inputs(cfg, min(B, 64), frames=T, seed=seed)
    rep = (B + 63) // 64
    a = small["audio_emb"].repeat(rep, 1, 1)[:B].cuda().contiguous()
    h = small["pretrain_aud_feat"].repeat(rep, 1, 1)[:B].cuda().contiguous()
    p = torch.zeros(B, cfg.style_dim, device="cuda:0")
    p[torch.arange(B), torch.arange(B) % cfg.style_dim] = 1.0
    return a, p, {"pretrain_aud_feat": h}


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def evaluations(tr, masked):
    d = tr.diffusion_ddim_val
    o = d._opts(0, False, 1, 0)
    spec = _lib.run_spec(timesteps=d._kept or (), masked=int(masked))
    steps, draws = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().dsh_sample_count(C.byref(o), C.byref(spec), C.byref(draws), C.byref(steps)), "dsh_sample_count")
    steps, draws = steps.value, draws.value
    return int(steps) if not masked else int(draws - 1 - steps)          # masked: draws = 1 + 2 evaluations + undo steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=950)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    cfg = get_config("show")
    model = UniDiffuser(cfg, make_synthetic_state_dict(cfg, 1234), device="cuda:0", precision="bf16")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    T, Cc, L = cfg.n_poses, cfg.net_dim_pose, cfg.overlap_len
    big, one, two = inputs(cfg, args.batch, T, 19), inputs(cfg, 1, T, 20), inputs(cfg, 2, T, 21)
    gt = torch.zeros(1, T, Cc, device="cuda:0")
    gt[:, :L] = torch.randn(1, L, Cc, generator=torch.Generator().manual_seed(5)).cuda()
    mask = torch.zeros(1, T, Cc, dtype=torch.bool, device="cuda:0")
    mask[:, :L] = True
    window = {"gt": gt, "outpainting_mask": mask, "outpainting_mask_any": True}

    tr.set_sampling(250, "ddim", "ddim")
    x250 = tr.generate_batch(two[0], two[1], Cc, two[2], {}, seed=77).clone()
    rows, base = [], None
    for steps, spacing, solver in CONFIGS:
        tr.set_sampling(steps, spacing, solver)
        r = {"steps": steps, "spacing": spacing, "solver": solver, "evaluations": evaluations(tr, False),
             "window_evaluations": evaluations(tr, True)}
        t_big = timed(lambda: tr.generate_batch(big[0], big[1], Cc, big[2], {}, seed=11), args.warmup, args.steps)
        t_one = timed(lambda: tr.generate_batch(one[0], one[1], Cc, one[2], {}, seed=11), args.warmup + 1, 5 * args.steps)
        t_win = timed(lambda: tr.generate_batch(one[0], one[1], Cc, one[2], dict(window), seed=11), args.warmup + 1, 5 * args.steps)
        x = tr.generate_batch(two[0], two[1], Cc, two[2], {}, seed=77)
        r.update(batch=args.batch, batch_frames_per_s=args.batch * T / t_big, batch_ms=1e3 * t_big, clip_frames_per_s=T / t_one,
                 clip_ms=1e3 * t_one, window_frames_per_s=(T - L) / t_win, window_ms=1e3 * t_win,
                 dist_to_ddim250=float((x - x250).abs().max() / x250.abs().max()))
        base = base or r
        r.update(batch_speedup=base["batch_ms"] / r["batch_ms"], expected_speedup=base["evaluations"] / r["evaluations"],
                 window_speedup=base["window_ms"] / r["window_ms"],
                 expected_window_speedup=base["window_evaluations"] / r["window_evaluations"])
        rows.append(r)
        print(json.dumps(r), flush=True)
    print(json.dumps({"summary": [[f"{r['steps']}/{r['spacing']}/{r['solver']}", round(r["batch_frames_per_s"]), round(r["batch_speedup"], 2),
                                   round(r["dist_to_ddim250"], 4)] for r in rows]}))


if __name__ == "__main__":
    main()
