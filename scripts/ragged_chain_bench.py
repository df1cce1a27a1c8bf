#!/usr/bin/env python3
"""What sampling chains of different lengths TOGETHER buys on a multi-chain stream: bench.py's --mode chain workload (SHOW, 9000 frames,
32 chains, bf16, ddim25, jump (3,5), CFG at the config's cond_scale) through ``sample_arbitrary_len_sharded`` with ``ragged`` off (one
chain batch per distinct segment length, one after another) and on (one ragged chain batch), alternated in ONE process, every pass
timed with device events after a warm-up pass of each mode.

usage: python scripts/ragged_chain_bench.py [--rounds 5] [--chains 32] [--stream-frames 9000] [--precision bf16]
Prints the per-pass times, then frames/s (median) and the number of sequential windows for both modes, and the ratio."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.model import UniDiffuser  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace, split_segments, window_lengths  # noqa: E402
from diffsheg_amd.weights import make_synthetic_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="off / on pairs after the warm-up (>= 3)")
    ap.add_argument("--chains", type=int, default=32)
    ap.add_argument("--stream-frames", type=int, default=9000)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--max-chains-per-batch", type=int, default=64)
    args = ap.parse_args()
    assert args.rounds >= 3
    cfg = get_config("show")
    model = UniDiffuser(cfg, make_synthetic_state_dict(cfg, 1234), device="cuda:0", precision=args.precision)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    N = args.stream_frames
    inp = make_inputs(cfg, 1, frames=N, seed=3)
    audio, hubert, pid = inp["audio_emb"].cuda(), inp["pretrain_aud_feat"].cuda(), inp["person_id"].cuda()
    segs = split_segments(N, args.chains, cfg.n_poses, cfg.overlap_len)
    step, mc = cfg.n_poses - cfg.overlap_len, args.max_chains_per_batch
    nwin = lambda n: len(window_lengths(n, cfg.n_poses, step))
    by_len = {}
    for s in segs:
        by_len[len(s)] = by_len.get(len(s), 0) + 1
    seq_off = sum(nwin(n) * ((c + mc - 1) // mc) for n, c in by_len.items())
    seq_on = sum(max(nwin(len(s)) for s in segs[c0:c0 + mc]) for c0 in range(0, len(segs), mc))

    def run(i, ragged):
        model._cond_key = None                       # a fresh stream every pass, as bench.py's step does
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = tr.sample_arbitrary_len_sharded(audio, pid, {"pretrain_aud_feat": hubert}, args.chains, seed=2024 + 7919 * i,
                                              max_chains_per_batch=mc, ragged=ragged)
        e1.record()
        e1.synchronize()
        assert tuple(out.shape) == (1, N, cfg.net_dim_pose) and torch.isfinite(out).all()
        return e0.elapsed_time(e1)

    for ragged in (False, True):
        run(-1, ragged)
    ms = {False: [], True: []}
    for i in range(args.rounds):
        for ragged in (False, True):
            ms[ragged].append(run(i, ragged))
        print(f"round {i}: ragged off {ms[False][-1]:8.1f} ms   on {ms[True][-1]:8.1f} ms", flush=True)
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    print(f"SHOW {args.precision} ddim25 jump ({cfg.jump_length},{cfg.jump_n_sample}) cond_scale {cfg.cond_scale}: {N} frames, {len(segs)} chains: "
          + ", ".join(f"{c} x {n} frames" for n, c in sorted(by_len.items(), reverse=True)))
    print(f"ragged off: {N / off * 1e3:9.1f} frames/s  (median {off:.1f} ms, min {min(ms[False]):.1f}, max {max(ms[False]):.1f}; {seq_off} sequential windows)")
    print(f"ragged on : {N / on * 1e3:9.1f} frames/s  (median {on:.1f} ms, min {min(ms[True]):.1f}, max {max(ms[True]):.1f}; {seq_on} sequential windows)")
    print(f"off / on time ratio (speed-up): {off / on:.3f}")


if __name__ == "__main__":
    main()
