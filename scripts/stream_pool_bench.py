#!/usr/bin/env python3
"""What batching live sessions buys: S SHOW sessions (bf16, ddim25, jump (3,5), CFG at the config's cond_scale) in one
``StreamPool``, all with a CHAINED window due at the same moment, against the only thing a caller had before the pool: S sequential
B = 1 chained windows of ``sample_arbitrary_len`` (one chain of its own per session).

For every S in --sessions: sessions are opened, their first window is taken, then every timed round feeds one stride
(``step_len = n_poses - overlap_len`` frames) to each and times ONE ``pool.step()`` with device events (it ends in the sampler's own
end-of-call synchronisation).  The sequential figure times, per round, S two-window chains ``sample_arbitrary_len([1, n_poses +
step_len])`` minus S one-window chains ``[1, n_poses]`` (the chained window alone, its plain first window subtracted), alternated with
the pool rounds in the same process.

usage: python scripts/stream_pool_bench.py [--sessions 1 8 32 128] [--rounds 5] [--precision bf16] [--fps 30]
Prints per S: the step() time (median, min, max), frames/s, the sequential time and the ratio; then the largest measured S whose step()
stays below step_len / fps seconds — the sessions one GPU sustains at that frame rate.  Nothing is gated on a time."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.model import UniDiffuser  # noqa: E402
from diffsheg_amd.streaming import StreamPool  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from diffsheg_amd.weights import make_synthetic_state_dict  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds per session count, after one warm-up round (>= 3)")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--sequential-cap", type=int, default=32, help="sequential B = 1 windows timed per round (scaled up to S)")
    args = ap.parse_args()
    assert args.rounds >= 3
    cfg = get_config("show")
    model = UniDiffuser(cfg, make_synthetic_state_dict(cfg, 1234), device="cuda:0", precision=args.precision)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    size, st, Cc = cfg.n_poses, cfg.n_poses - cfg.overlap_len, cfg.net_dim_pose
    budget_ms = st / args.fps * 1e3
    n_frames = size + (args.rounds + 1) * st
    results = []
    for S in args.sessions:
        inp = make_inputs(cfg, min(S, 64), frames=n_frames, seed=11)
        audio = inp["audio_emb"].cuda().repeat((S + 63) // 64, 1, 1)[:S]
        hubert = inp["pretrain_aud_feat"].cuda().repeat((S + 63) // 64, 1, 1)[:S]
        pid = torch.zeros(S, cfg.style_dim, device="cuda:0")
        pid[torch.arange(S), torch.arange(S) % cfg.style_dim] = 1.0
        pool = StreamPool(tr, S, seed=2024)
        sids = [pool.open(pid[b], key=b) for b in range(S)]
        for b, sid in enumerate(sids):
            pool.feed(sid, audio[b, :size], {"pretrain_aud_feat": hubert[b, :size]})
        assert len(pool.step()) == S                     # the first windows (plain schedule): not what is measured
        n_seq = min(S, args.sequential_cap)

        def pool_round(r):
            for b, sid in enumerate(sids):
                lo = size + r * st
                pool.feed(sid, audio[b, lo:lo + st], {"pretrain_aud_feat": hubert[b, lo:lo + st]})
            ms, out = timed(pool.step)
            assert len(out) == S and all(tuple(t.shape) == (st, Cc) for t in out.values())
            return ms

        def seq_round(r):
            def chains(frames):
                for b in range(n_seq):
                    model._cond_key = None
                    tr.sample_arbitrary_len(audio[b:b + 1, :frames], pid[b:b + 1], {"pretrain_aud_feat": hubert[b:b + 1, :frames]},
                                            seed=2024 + r, row_keys=[b])
            two, _ = timed(lambda: chains(size + st))
            one, _ = timed(lambda: chains(size))
            return (two - one) * S / n_seq

        pool_round(0)
        seq_round(0)
        p_ms, s_ms = [], []
        for r in range(1, args.rounds + 1):
            p_ms.append(pool_round(r))
            s_ms.append(seq_round(r))
            print(f"S={S:4d} round {r}: pool.step() {p_ms[-1]:9.2f} ms   {S} sequential B=1 chained windows {s_ms[-1]:9.2f} ms", flush=True)
        pool.close_many(sids)
        pm, sm = statistics.median(p_ms), statistics.median(s_ms)
        results.append((S, pm))
        print(f"S={S:4d}: step() median {pm:.2f} ms (min {min(p_ms):.2f}, max {max(p_ms):.2f}) = {S * st / pm * 1e3:9.1f} frames/s; "
              f"sequential median {sm:.2f} ms = {S * st / sm * 1e3:9.1f} frames/s"
              f"{'' if n_seq == S else f' (from {n_seq} windows, scaled)'}; sequential / pool {sm / pm:.2f}; "
              f"real-time budget at {args.fps:g} fps {budget_ms:.0f} ms: {'inside' if pm < budget_ms else 'OUTSIDE'}", flush=True)
    ok = [S for S, pm in results if pm < budget_ms]
    print(f"SHOW {args.precision} ddim25 jump ({cfg.jump_length},{cfg.jump_n_sample}) cond_scale {cfg.cond_scale}: largest measured S whose step() stays "
          f"below step_len / fps = {budget_ms:.0f} ms: {max(ok) if ok else 'none'} sessions per GPU at {args.fps:g} fps")


if __name__ == "__main__":
    main()
