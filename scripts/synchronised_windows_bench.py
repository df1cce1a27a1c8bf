#!/usr/bin/env python3
"""One long stream three ways (SHOW, bf16, ddim25, CFG at the config's cond_scale): the sequential window chain
(``sample_arbitrary_len``), ``--chains`` independent chains with seam repair (``sample_arbitrary_len_sharded(seam_repair=True)``, as
scripts/seam_repair_bench.py runs them) and the synchronised window batch (``sample_arbitrary_len_synchronised``), alternated in ONE
process, every pass timed with device events after a warm-up round, medians of ``--rounds``.

Also: the synchronised batch with the reconciliation launch doing nothing (``sync_left`` all -1: the same single chain and launches, no
shared frames), which prices the launch; and one stream of ``--long-windows`` windows, long enough to cross the sub-batch split limit,
as the synchronised single chain and as the plain loop's free-running sub-batch streams on the same batch, which prices the
single-chain rule.

usage: python scripts/synchronised_windows_bench.py [--rounds 5] [--chains 32] [--stream-frames 9000] [--long-windows 400]
       [--precision bf16] [--skip-chain]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.model import UniDiffuser  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace, synchronised_window_plan  # noqa: E402
from diffsheg_amd.weights import make_synthetic_state_dict  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def window_batch(tr, cfg, audio, hubert, pid, seed):
    """the synchronised batch of one stream as ddim_sample_loop arguments: (shape, x_T, model_kwargs, left)"""
    N = int(audio.shape[1])
    plan = synchronised_window_plan([N], cfg.n_poses, cfg.overlap_len)
    rows, T = len(plan["left"]), plan["frames"]

    def cut(t):
        out = t.new_zeros((rows, T) + tuple(t.shape[2:]))
        for r, (st, n) in enumerate(zip(plan["start"], plan["lengths"])):
            out[r, :n] = t[0, st:st + n]
        return out
    z = tr.diffusion_ddim_val.draw_noise(1, N, cfg.net_dim_pose, audio.device, seed, [0])
    kw = {"audio_emb": cut(audio), "length": torch.tensor(plan["lengths"]), "person_id": pid.expand(rows, -1).contiguous(),
          "add_cond": {"pretrain_aud_feat": cut(hubert)}, "y": {}, "pe_type": "pe_sinu"}
    return (rows, T, cfg.net_dim_pose), cut(z), kw, plan["left"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chains", type=int, default=32)
    ap.add_argument("--stream-frames", type=int, default=9000)
    ap.add_argument("--long-windows", type=int, default=400, help="windows of the stream that crosses the split limit (0: skip)")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--skip-chain", action="store_true", help="leave the sequential chain out (seconds per pass)")
    args = ap.parse_args()
    cfg = get_config("show")
    model = UniDiffuser(cfg, make_synthetic_state_dict(cfg, 1234), device="cuda:0", precision=args.precision)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    dd = tr.diffusion_ddim_val
    N, L = args.stream_frames, cfg.overlap_len
    inp = make_inputs(cfg, 1, frames=N, seed=3)
    audio, hubert, pid = inp["audio_emb"].cuda(), inp["pretrain_aud_feat"].cuda(), inp["person_id"].cuda()
    cond = {"pretrain_aud_feat": hubert}
    shape, xT, kw, left = window_batch(tr, cfg, audio, hubert, pid, 2024)

    def loop(shape, xT, kw, **more):
        return dd.ddim_sample_loop(model, shape, noise=xT, clip_denoised=False, model_kwargs=kw, seed=1, **more)
    paths = {
        "chain": lambda i: tr.sample_arbitrary_len(audio, pid, cond, seed=2024 + 7919 * i),
        "chains+repair": lambda i: tr.sample_arbitrary_len_sharded(audio, pid, cond, args.chains, seed=2024 + 7919 * i, seam_repair=True),
        "synchronised": lambda i: tr.sample_arbitrary_len_synchronised(audio, pid, cond, seed=2024 + 7919 * i),
        "sync loop only": lambda i: loop(shape, xT, kw, sync_left=left, sync_len=L),
        "sync loop, no shared frames": lambda i: loop(shape, xT, kw, sync_left=[-1] * len(left), sync_len=L),
    }
    if args.skip_chain:
        del paths["chain"]
    ms = {k: [] for k in paths}
    for i in range(-1, args.rounds):
        for name, fn in paths.items():
            model._cond_key = None                   # a fresh stream every pass, as bench.py's step does
            t, out = timed(lambda: fn(i))
            assert torch.isfinite(out).all()
            if i >= 0:
                ms[name].append(t)
        if i >= 0:
            print(f"round {i}: " + "   ".join(f"{k} {v[-1]:.1f} ms" for k, v in ms.items()), flush=True)
    print(f"SHOW {args.precision} ddim25 cond_scale {cfg.cond_scale}: one stream of {N} frames = {shape[0]} windows of {shape[1]} frames, overlap {L}")
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        print(f"{k:30s} {N / med[k] * 1e3:10.1f} frames/s  (median {med[k]:.1f} ms, min {min(v):.1f}, max {max(v):.1f})")
    d = med["sync loop only"] - med["sync loop, no shared frames"]
    print(f"reconciliation of the shared frames: {d * 1e3 / 25:.1f} us per step over 25 steps (difference of the two loop medians; both issue the launch)")
    if "chain" in med:
        print(f"synchronised vs chain: x {med['chain'] / med['synchronised']:.1f}")
    print(f"synchronised vs {args.chains} chains + repair: x {med['chains+repair'] / med['synchronised']:.2f}")
    if args.long_windows <= 0:
        return
    # one stream across the split limit: the synchronised single chain against the plain loop's free-running sub-batch streams
    from diffsheg_amd import _lib
    NL = cfg.n_poses + (args.long_windows - 1) * (cfg.n_poses - L)
    inp = make_inputs(cfg, 1, frames=NL, seed=5)
    a2, h2 = inp["audio_emb"].cuda(), inp["pretrain_aud_feat"].cuda()
    shape2, xT2, kw2, left2 = window_batch(tr, cfg, a2, h2, pid, 7)
    long_paths = {"synchronised (one chain)": dict(sync_left=left2, sync_len=L), "plain loop (sub-batch streams)": {}}
    ms2, streams = {k: [] for k in long_paths}, {}
    for i in range(-1, args.rounds):
        for name, more in long_paths.items():
            model._cond_key = None
            _lib.launch_counts(reset=True)
            t, out = timed(lambda: loop(shape2, xT2, kw2, **more))
            streams[name] = _lib.launch_counts()["sample_streams"]
            assert torch.isfinite(out).all()
            if i >= 0:
                ms2[name].append(t)
    print(f"one stream of {NL} frames = {shape2[0]} windows ({shape2[0] * shape2[1]} token rows):")
    for k, v in ms2.items():
        m = statistics.median(v)
        print(f"{k:30s} {NL / m * 1e3:10.1f} frames/s  (median {m:.1f} ms, min {min(v):.1f}, max {max(v):.1f}; {streams[k]} sampling stream(s))")


if __name__ == "__main__":
    main()
