#!/usr/bin/env python3
"""What soft constraints cost per sampled clip: ``generate_batch`` on the SHOW ddim25 workload (CFG at the config's cond_scale) unguided,
with the attraction term alone and with all three terms (``glue.MotionGuidance``, both spaces), B = 1 / 100 / 950 clips — in ONE
process, the variants alternated in rotating order, every step timed with device events after one warm-up step of each.  By bytes
the guided step kernel reads two more [B, T, C] tensors beside the four its parent moves, against an evaluation that dominates; its
mapping (one lane per column of a clip, walking the frames) has less parallelism than the parent's at small batch.  Compare figures
inside one run of this script only.

usage: python scripts/guidance_bench.py [--steps 5] [--precision bf16] [--batches 1,100,950] [--space x0]
Prints every step's time, then per batch the median of each variant, its difference to the unguided median and that difference per
denoise step (25)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.glue import MotionGuidance  # noqa: E402
from diffsheg_amd.model import UniDiffuser  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from diffsheg_amd.weights import make_synthetic_state_dict  # noqa: E402

MODES = ("unguided", "attraction", "all three")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="timed steps of every variant after its warm-up step")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--batches", default="1,100,950")
    ap.add_argument("--space", default="x0", choices=["x0", "x_t"])
    args = ap.parse_args()
    cfg = get_config("show")
    dev = "cuda:0"
    model = UniDiffuser(cfg, make_synthetic_state_dict(cfg, 1234), device=dev, precision=args.precision)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    T, Cc = cfg.n_poses, cfg.net_dim_pose
    summary = []
    for B in (int(b) for b in args.batches.split(",")):
        small = make_inputs(cfg, min(B, 64), seed=3)
        rep = (B + 63) // 64
        audio, hubert, pid = (small[k].repeat(rep, 1, 1)[:B].cuda().contiguous() if small[k].dim() == 3 else small[k].repeat(rep, 1)[:B].cuda().contiguous()
                              for k in ("audio_emb", "pretrain_aud_feat", "person_id"))
        gen = torch.Generator(device=dev).manual_seed(7)
        Y = torch.randn(B, T, Cc, device=dev, generator=gen)
        W = torch.zeros(B, T, Cc, device=dev)
        W[:, ::11, :90] = 0.2                                # a keyframe on the body and hand columns every 11 frames
        vel, acc = torch.full((Cc,), 0.03, device=dev), torch.full((Cc,), 0.01, device=dev)
        guides = {"unguided": None, "attraction": MotionGuidance(Y, W, space=args.space),
                  "all three": MotionGuidance(Y, W, vel, acc, space=args.space)}

        def run(i, mode):
            model._cond_key = None                           # conditioned afresh every step, as bench.py's step is
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = tr.generate_batch(audio, pid, Cc, {"pretrain_aud_feat": hubert}, {}, seed=2024 + 7919 * i, guidance=guides[mode])
            e1.record()
            e1.synchronize()
            assert tuple(out.shape) == (B, T, Cc) and torch.isfinite(out).all()
            return e0.elapsed_time(e1)

        for mode in MODES:
            run(-1, mode)
        ms = {m: [] for m in MODES}
        for i in range(args.steps):
            r = i % len(MODES)
            order = MODES[r:] + MODES[:r]
            for mode in order:
                ms[mode].append(run(i, mode))
            print(f"B={B:>4} step {i} (order {' > '.join(order)}): " + "   ".join(f"{m} {ms[m][-1]:9.2f} ms" for m in MODES), flush=True)
        med = {m: statistics.median(ms[m]) for m in MODES}
        summary.append(f"{B:>5} clip(s): " + "   ".join(f"{m} {med[m]:9.2f} ms" for m in MODES) + "   extra: " +
                       "  ".join(f"{m} {med[m] - med['unguided']:+.2f} ms = {(med[m] - med['unguided']) / 25 * 1e3:+.1f} us per step "
                                 f"({(med[m] / med['unguided'] - 1) * 100:+.2f} %)" for m in MODES[1:]))
    print(f"SHOW {args.precision} ddim25 T = {T}, CFG {cfg.cond_scale}, guidance space {args.space}; median of {args.steps} timed steps each:")
    for line in summary:
        print(line)


if __name__ == "__main__":
    main()
