#!/usr/bin/env python3
"""What sampling ONE modality costs next to the joint run: ``modality="both"`` / ``"expression"`` / ``"gesture"`` (the latter with a
seeded given track) on four shapes of the SHOW ddim25 workload with CFG at the config's cond_scale — the 950-clip batch of bench.py, 100
clips, a single clip (a chain's first window) and a single chained window (out-painting mask, jump (3,5): 63 evaluations) — in ONE
process, the three modes alternated in rotating order, every step timed with device events after one warm-up step of each mode.
Compare figures inside one run of this script only.

usage: python scripts/modality_bench.py [--steps 3] [--precision bf16] [--shapes 950,100,1,chained]
Prints every step's time, then per shape the median of each mode and the joint / partial time ratios."""
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

MODES = ("both", "expression", "gesture")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="timed steps of every mode after its warm-up step")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--shapes", default="950,100,1,chained")
    args = ap.parse_args()
    cfg = get_config("show")
    model = UniDiffuser(cfg, make_synthetic_state_dict(cfg, 1234), device="cuda:0", precision=args.precision)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    T, Cc, L = cfg.n_poses, cfg.net_dim_pose, cfg.overlap_len
    summary = []
    for shape in args.shapes.split(","):
        B = 1 if shape == "chained" else int(shape)
        small = make_inputs(cfg, min(B, 64), seed=3)
        rep = (B + 63) // 64
        audio, hubert, pid = (small[k].repeat(rep, 1, 1)[:B].cuda().contiguous() if small[k].dim() == 3 else small[k].repeat(rep, 1)[:B].cuda().contiguous()
                              for k in ("audio_emb", "pretrain_aud_feat", "person_id"))
        g = torch.Generator(device="cuda:0").manual_seed(7)
        track = torch.randn(B, T, cfg.expression_dim, device="cuda:0", generator=g)
        y = {}
        if shape == "chained":
            gt = torch.zeros(B, T, Cc, device="cuda:0")
            gt[:, :L] = torch.randn(B, L, Cc, device="cuda:0", generator=g)
            mask = torch.zeros(B, T, Cc, dtype=torch.bool, device="cuda:0")
            mask[:, :L] = True
            y = {"gt": gt, "outpainting_mask": mask, "outpainting_mask_any": True}

        def run(i, mode):
            model._cond_key = None                       # conditioned afresh every step, as bench.py's step is
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = tr.generate_batch(audio, pid, Cc, {"pretrain_aud_feat": hubert}, dict(y), seed=2024 + 7919 * i, modality=mode,
                                    expression=track if mode == "gesture" else None)
            e1.record()
            e1.synchronize()
            assert tuple(out.shape) == (B, T, Cc) and torch.isfinite(out).all()
            return e0.elapsed_time(e1)

        for mode in MODES:
            run(-1, mode)
        ms = {m: [] for m in MODES}
        for i in range(args.steps):
            order = MODES[i % 3:] + MODES[:i % 3]
            for mode in order:
                ms[mode].append(run(i, mode))
            print(f"{shape:>8} step {i} (order {' > '.join(order)}): " + "   ".join(f"{m} {ms[m][-1]:9.2f} ms" for m in MODES), flush=True)
        med = {m: statistics.median(ms[m]) for m in MODES}
        summary.append(f"{'chained window, 1 clip' if shape == 'chained' else shape + ' clip(s)':>24}: " +
                       "   ".join(f"{m} {med[m]:9.2f} ms" for m in MODES) +
                       f"   joint / expression {med['both'] / med['expression']:.3f}   joint / gesture {med['both'] / med['gesture']:.3f}")
    print(f"SHOW {args.precision} ddim25 T = {T}, CFG {cfg.cond_scale}; median of {args.steps} timed steps per mode:")
    for line in summary:
        print(line)


if __name__ == "__main__":
    main()
