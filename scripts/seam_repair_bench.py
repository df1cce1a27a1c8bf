#!/usr/bin/env python3
"""Cost of closing the seams of a multi-chain stream: bench.py's --mode chain workload (SHOW, 9000 frames, 32 chains, bf16,
ddim25, jump (3,5), CFG at the config's cond_scale) through ``sample_arbitrary_len_sharded`` with ``seam_repair`` off and on,
alternated in ONE process, every pass timed with device events after a warm-up pass of each mode.

usage: python scripts/seam_repair_bench.py [--rounds 5] [--chains 32] [--stream-frames 9000] [--precision bf16]
Prints the per-pass times, then frames/s (median) for both modes and the ratio."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.model import UniDiffuser  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace, split_segments_for_repair  # noqa: E402
from diffsheg_amd.weights import make_synthetic_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="off / on pairs after the warm-up (>= 3)")
    ap.add_argument("--chains", type=int, default=32)
    ap.add_argument("--stream-frames", type=int, default=9000)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args()
    assert args.rounds >= 3
    cfg = get_config("show")
    model = UniDiffuser(cfg, make_synthetic_state_dict(cfg, 1234), device="cuda:0", precision=args.precision)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    N = args.stream_frames
    inp = make_inputs(cfg, 1, frames=N, seed=3)
    audio, hubert, pid = inp["audio_emb"].cuda(), inp["pretrain_aud_feat"].cuda(), inp["person_id"].cuda()
    segs = split_segments_for_repair(N, args.chains, cfg.n_poses, cfg.overlap_len)

    def run(i, repair):
        model._cond_key = None                       # a fresh stream every pass, as bench.py's step does
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = tr.sample_arbitrary_len_sharded(audio, pid, {"pretrain_aud_feat": hubert}, args.chains, seed=2024 + 7919 * i,
                                              seam_repair=repair)
        e1.record()
        e1.synchronize()
        assert tuple(out.shape) == (1, N, cfg.net_dim_pose) and torch.isfinite(out).all()
        return e0.elapsed_time(e1)

    for repair in (False, True):
        run(-1, repair)
    ms = {False: [], True: []}
    for i in range(args.rounds):
        for repair in (False, True):
            ms[repair].append(run(i, repair))
        print(f"round {i}: seam_repair off {ms[False][-1]:8.1f} ms   on {ms[True][-1]:8.1f} ms", flush=True)
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    print(f"SHOW {args.precision} ddim25 jump ({cfg.jump_length},{cfg.jump_n_sample}) cond_scale {cfg.cond_scale}: {N} frames, "
          f"{len(segs)} chains of {min(map(len, segs))} - {max(map(len, segs))} frames, {len(segs) - 1} seams as one batched window")
    print(f"seam_repair off: {N / off * 1e3:9.1f} frames/s  (median {off:.1f} ms, min {min(ms[False]):.1f}, max {max(ms[False]):.1f})")
    print(f"seam_repair on : {N / on * 1e3:9.1f} frames/s  (median {on:.1f} ms, min {min(ms[True]):.1f}, max {max(ms[True]):.1f})")
    print(f"on / off time ratio: {on / off:.3f}   (repair pass: {on - off:.1f} ms)")


if __name__ == "__main__":
    main()
