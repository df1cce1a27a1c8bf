#!/usr/bin/env python3
"""What a guidance schedule costs per sampled clip: ``generate_batch`` on the SHOW ddim25 workload (CFG at the config's cond_scale)
unscheduled, with gains only (``glue.CFGSchedule``: one scheduled mix launch per encoder and evaluation in place of the plain one) and
with gains + std rescale (two launches per encoder and evaluation), B = 1 / 100 / 950 clips — in ONE process, the variants alternated in
rotating order, every step timed with device events after one warm-up step of each.  By launches, gains only changes nothing and the
rescale adds two small launches per evaluation (50 per ddim25 loop, where the loop is not replayed from a graph); by bytes the rescale
re-reads the conditional prediction and eps of its own encoder once and moves 32 bytes of moments per token row.  Compare figures inside
one run of this script only.

usage: python scripts/cfg_schedule_bench.py [--steps 5] [--precision bf16] [--batches 1,100,950]
Prints every step's time, then per batch the median of each variant and its difference to the unscheduled median."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.glue import CFGSchedule  # noqa: E402
from diffsheg_amd.model import UniDiffuser  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from diffsheg_amd.weights import make_synthetic_state_dict  # noqa: E402

MODES = ("unscheduled", "gains only", "gains + rescale")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="timed steps of every variant after its warm-up step")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32", "bf16x3"])
    ap.add_argument("--batches", default="1,100,950")
    args = ap.parse_args()
    cfg = get_config("show")
    dev = "cuda:0"
    model = UniDiffuser(cfg, make_synthetic_state_dict(cfg, 1234), device=dev, precision=args.precision)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    T, Cc = cfg.n_poses, cfg.net_dim_pose
    ramp = lambda t: 0.25 + 1.5 * t / 999.0                  # (no gain is 1: every clip takes the general branch of the mix)
    scheds = {"unscheduled": None, "gains only": CFGSchedule(ramp, lambda t: 2.0 - ramp(t)),
              "gains + rescale": CFGSchedule(ramp, lambda t: 2.0 - ramp(t), rescale=(0.7, 0.3))}
    summary = []
    for B in (int(b) for b in args.batches.split(",")):
        small = make_inputs(cfg, min(B, 64), seed=3)
        rep = (B + 63) // 64
        audio, hubert, pid = (small[k].repeat(rep, 1, 1)[:B].cuda().contiguous() if small[k].dim() == 3 else small[k].repeat(rep, 1)[:B].cuda().contiguous()
                              for k in ("audio_emb", "pretrain_aud_feat", "person_id"))

        def run(i, mode):
            model._cond_key = None                           # conditioned afresh every step, as bench.py's step is
            model.set_guidance_schedule(scheds[mode])        # (sticky, outside the timed region: what a user sets once)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = tr.generate_batch(audio, pid, Cc, {"pretrain_aud_feat": hubert}, {}, seed=2024 + 7919 * i)
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
                       "  ".join(f"{m} {med[m] - med['unscheduled']:+.2f} ms = {(med[m] - med['unscheduled']) / 25 * 1e3:+.1f} us per evaluation "
                                 f"({(med[m] / med['unscheduled'] - 1) * 100:+.2f} %)" for m in MODES[1:]))
    model.set_guidance_schedule(None)
    print(f"SHOW {args.precision} ddim25 T = {T}, CFG {cfg.cond_scale}; median of {args.steps} timed steps each:")
    for line in summary:
        print(line)


if __name__ == "__main__":
    main()
