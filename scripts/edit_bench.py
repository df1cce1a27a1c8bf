#!/usr/bin/env python3
"""What a variation of an existing motion costs next to a clip sampled from noise: ``DDPMTrainer.sample_variations`` at start levels
K = 5 / 10 / 25 (q_sample + K DDIM steps in one native call) against ``generate_batch`` (25 steps from noise) on the SHOW ddim25
workload with CFG at the config's cond_scale, B = 1 and B = 100 clips — in ONE process, the four alternated in rotating order, every
step timed with device events after one warm-up step of each.  The expectation to test: a variation at K costs about K / 25 of a clip
from noise.  Compare figures inside one run of this script only.

usage: python scripts/edit_bench.py [--steps 5] [--precision bf16] [--batches 1,100] [--levels 5,10,25]
Prints every step's time, then per batch the median of each and its ratio to the from-noise clip."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.model import UniDiffuser  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from diffsheg_amd.weights import make_synthetic_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="timed steps of every variant after its warm-up step")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--batches", default="1,100")
    ap.add_argument("--levels", default="5,10,25")
    args = ap.parse_args()
    cfg = get_config("show")
    model = UniDiffuser(cfg, make_synthetic_state_dict(cfg, 1234), device="cuda:0", precision=args.precision)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    T, Cc = cfg.n_poses, cfg.net_dim_pose
    levels = [int(k) for k in args.levels.split(",")]
    modes = ["noise"] + [f"K={k}" for k in levels]
    summary = []
    for B in (int(b) for b in args.batches.split(",")):
        small = make_inputs(cfg, min(B, 64), seed=3)
        rep = (B + 63) // 64
        audio, hubert, pid = (small[k].repeat(rep, 1, 1)[:B].cuda().contiguous() if small[k].dim() == 3 else small[k].repeat(rep, 1)[:B].cuda().contiguous()
                              for k in ("audio_emb", "pretrain_aud_feat", "person_id"))
        motions = torch.randn(B, T, Cc, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(7))

        def run(i, mode):
            model._cond_key = None                       # conditioned afresh every step, as bench.py's step is
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if mode == "noise":
                out = tr.generate_batch(audio, pid, Cc, {"pretrain_aud_feat": hubert}, {}, seed=2024 + 7919 * i)
            else:
                out = tr.sample_variations(motions, audio, pid, {"pretrain_aud_feat": hubert}, level=int(mode[2:]), seed=2024 + 7919 * i)
            e1.record()
            e1.synchronize()
            assert tuple(out.shape) == (B, T, Cc) and torch.isfinite(out).all()
            return e0.elapsed_time(e1)

        for mode in modes:
            run(-1, mode)
        ms = {m: [] for m in modes}
        for i in range(args.steps):
            r = i % len(modes)
            order = modes[r:] + modes[:r]
            for mode in order:
                ms[mode].append(run(i, mode))
            print(f"B={B:>4} step {i} (order {' > '.join(order)}): " + "   ".join(f"{m} {ms[m][-1]:9.2f} ms" for m in modes), flush=True)
        med = {m: statistics.median(ms[m]) for m in modes}
        summary.append(f"{B:>5} clip(s): " + "   ".join(f"{m} {med[m]:9.2f} ms" for m in modes) + "   ratio to noise: " +
                       "  ".join(f"{m} {med[m] / med['noise']:.3f} (K/25 = {int(m[2:]) / 25:.2f})" for m in modes[1:]))
    print(f"SHOW {args.precision} ddim25 T = {T}, CFG {cfg.cond_scale}; median of {args.steps} timed steps each:")
    for line in summary:
        print(line)


if __name__ == "__main__":
    main()
