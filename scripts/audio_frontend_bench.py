#!/usr/bin/env python3
"""What the audio front costs in front of the sampler: hubert-large widths and depth with seeded weights, a 60 s and a 600 s
16 kHz signal.

  (a) AudioFrontEnd.features(), split into resampling + mel / HuBERT convolution stack (+ projection and positional convolution) / the 24
      transformer layers / interpolation to the mel frames.  The split of the encoder is taken from a second handle with 0 layers: what the
      full handle costs more is the layers;
  (b) what a user has without it: tests/hubert_ref.py in fp32 on the same GPU through torch (its `fast` form: torch's conv1d / matmul /
      scaled_dot_product_attention, chunk by chunk as the reference does), and transformers' HubertModel there if it is importable;
  (c) the time of sampling the same stream (sample_arbitrary_len, SHOW, ddim25).

--folder N adds the folder case: N utterances with durations spread evenly over 2 .. 15 s (in a seeded order), as one call of
AudioFrontEnd.features_batch (also with min_fill = 0.75: ragged passes of similar lengths) against the per-file loop over
AudioFrontEnd.features (the path before the batch form existed), and the sampling of the same batch (sample_arbitrary_len(.., lengths=));
the feature results are compared bit for bit.

--hubert-precision fp32,bf16 builds one encoder per precision in the same process and times them ALTERNATELY (round r of every precision
before round r + 1 of any), so that clock and pool drift hit both alike.  The first precision keeps the plain keys (features_ms, hubert_ms,
features_batch_ms, ..); every further one adds the same keys with its name as suffix (features_ms_bf16, ..) and, against the first one, the
largest and the rms feature difference as a fraction of the feature range and the difference of the sampled motion as a fraction of its range.

Prints one JSON line per signal length (and one for the folder); --out also writes them to a file.

Usage:  python scripts/audio_frontend_bench.py [--seconds 60,600] [--folder 32] [--repeat 3] [--precision bf16] [--hubert-precision fp32,bf16]
                                               [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hubert_ref  # noqa: E402
from diffsheg_amd import audio  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.model import UniDiffuser  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from diffsheg_amd.weights import make_synthetic_state_dict  # noqa: E402


def timed(fn, repeat: int) -> float:
    """median wall time of fn() in ms, synchronised on both sides, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def timed_alternately(fns: dict, repeat: int) -> dict:
    """median wall time in ms of every fns[name](), the names taking turns inside each round, after one warm-up call each"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(repeat):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: sorted(v)[len(v) // 2] for k, v in ts.items()}


def suffix(i: int, name: str) -> str:
    return "" if i == 0 else "_" + name


def feature_distance(a: torch.Tensor, b: torch.Tensor) -> tuple:
    """(max, rms) of a - b as fractions of b's range; lists of per-row results are compared as one tensor"""
    if isinstance(a, (list, tuple)):
        a, b = (torch.cat([t.reshape(-1, t.shape[-1]) for t in v]) for v in (a, b))
    rng = float(b.max() - b.min())
    d = (a - b).double()
    return float(d.abs().max()) / rng, float(d.pow(2).mean().sqrt()) / rng


def folder_precisions(fes: dict, tr, cfg, count: int, repeat: int) -> dict:
    """the folder's features_batch and the sampling behind it, once per encoder precision, timed alternately"""
    g = torch.Generator().manual_seed(count)
    secs = [2.0 + 13.0 * i / max(count - 1, 1) for i in torch.randperm(count, generator=g).tolist()]
    first = next(iter(fes.values()))
    waves = [(0.1 * torch.randn(int(16000 * s), generator=g)).to(first.device) for s in secs]
    pid = make_inputs(cfg, count, frames=cfg.n_poses, seed=3)["person_id"]
    feats = {k: fe.features_batch(waves) for k, fe in fes.items()}
    r = dict(zip(("features_batch_ms" + suffix(i, k) for i, k in enumerate(fes)),
                 timed_alternately({k: (lambda fe=fe: fe.features_batch(waves)) for k, fe in fes.items()}, repeat).values()))
    sample = lambda k: tr.sample_arbitrary_len(feats[k][0], pid, {"pretrain_aud_feat": feats[k][1]}, lengths=feats[k][2], seed=1)
    outs = {k: sample(k) for k in fes}
    base = next(iter(fes))
    for i, k in enumerate(fes):
        if i == 0:
            continue
        r["feature_max_over_range_" + k], r["feature_rms_over_range_" + k] = feature_distance(feats[k][1], feats[base][1])
        r["sample_max_over_range_" + k], r["sample_rms_over_range_" + k] = feature_distance(outs[k], outs[base])
        r["front_end_speedup_" + k] = r["features_batch_ms"] / r["features_batch_ms_" + k]
    return r


def folder_case(fe, tr, cfg, count: int, repeat: int, precision: str) -> dict:
    g = torch.Generator().manual_seed(count)
    secs = [2.0 + 13.0 * i / max(count - 1, 1) for i in torch.randperm(count, generator=g).tolist()]
    waves = [(0.1 * torch.randn(int(16000 * s), generator=g)).to(fe.device) for s in secs]
    loop = lambda: [fe.features(w) for w in waves]
    mel, hub, lengths = fe.features_batch(waves)
    same = all(torch.equal(mel[b, :n], m) and torch.equal(hub[b, :n], h) for b, (n, (m, h)) in enumerate(zip(lengths, loop())))
    pid = make_inputs(cfg, count, frames=cfg.n_poses, seed=3)["person_id"]
    r = {"folder": count, "seconds_min": min(secs), "seconds_max": max(secs), "seconds_total": sum(secs), "mel_frames_total": sum(lengths),
         "mel_frames_max": max(lengths), "batch_equals_loop_bitwise": same, "precision_sampler": precision}
    r["features_batch_ms"] = timed(lambda: fe.features_batch(waves), repeat)
    # the remainders in ragged passes of similar lengths (every one at least 3 / 4 of the longest of its pass) instead of one
    mel_g, hub_g, _ = fe.features_batch(waves, min_fill=0.75)
    r["grouped_passes"] = len(audio.length_groups([w.shape[0] for w in waves], 0.75))
    r["grouped_equals_batch_bitwise"] = torch.equal(mel_g, mel) and torch.equal(hub_g, hub)
    r["features_batch_grouped_ms"] = timed(lambda: fe.features_batch(waves, min_fill=0.75), repeat)
    r["features_loop_ms"] = timed(loop, repeat)
    r["loop_over_batch"] = r["features_loop_ms"] / r["features_batch_ms"]
    r["loop_over_batch_grouped"] = r["features_loop_ms"] / r["features_batch_grouped_ms"]
    r["sampling_ms"] = timed(lambda: tr.sample_arbitrary_len(mel, pid, {"pretrain_aud_feat": hub}, lengths=lengths, seed=1), repeat)
    return r


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", default="60,600")
    ap.add_argument("--folder", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--hubert-precision", default="fp32", help="comma-separated encoder precisions; the first one keeps the plain result keys")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "audio_frontend_bench needs a GPU"
    dev = "cuda:0"
    cfg_l = dict(hubert_ref.LARGE)
    sd = hubert_ref.make_state_dict(cfg_l, 1)
    precisions = [p for p in args.hubert_precision.split(",") if p]
    encs = {p: audio.HubertEncoder(cfg_l, device=dev, precision=p).load_state_dict(sd) for p in precisions}
    fes = {p: audio.AudioFrontEnd(e) for p, e in encs.items()}
    full = encs[precisions[0]]
    front = audio.HubertEncoder(dict(cfg_l, layers=0), device=dev).load_state_dict({k: v for k, v in sd.items() if not k.startswith("encoder.layers.")})
    fe = fes[precisions[0]]
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    cfg = get_config("show")
    model = UniDiffuser(cfg, make_synthetic_state_dict(cfg, 1234), device=dev, precision=args.precision)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    pid = make_inputs(cfg, 1, frames=cfg.n_poses, seed=3)["person_id"]
    hf = None
    try:
        from transformers import HubertConfig, HubertModel
        hc = HubertConfig(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, feat_extract_norm="layer",
                          conv_bias=True, do_stable_layer_norm=True, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16)
        hf = HubertModel(hc).eval().to(dev)
        hf.load_state_dict(sd, strict=False)
    except Exception as e:          # not installed on this machine
        print(f"# transformers' HubertModel not timed: {type(e).__name__}", file=sys.stderr)
    lines = []
    for sec in [int(s) for s in args.seconds.split(",") if s]:
        n = 16000 * sec
        wave = (0.1 * torch.randn(n, generator=torch.Generator().manual_seed(sec))).to(dev)
        norm = audio.normalize_wave(wave)
        w18 = audio.resample_poly(wave, 9, 8)
        mel, hub = fe.features(wave)
        rows = full.encode_long(wave)
        N = int(mel.shape[0])
        r = {"seconds": sec, "samples": n, "mel_frames": N, "hubert_rows": int(rows.shape[0]), "precision_sampler": args.precision,
             "hubert_precisions": precisions}
        r["features_ms"] = timed(lambda: fe.features(wave), args.repeat)
        if len(precisions) > 1:
            for key, call in (("features_ms", lambda p: fes[p].features(wave)), ("hubert_ms", lambda p: encs[p].encode_long(wave))):
                t = timed_alternately({p: (lambda p=p: call(p)) for p in precisions}, args.repeat)
                for i, p in enumerate(precisions):
                    r[key + suffix(i, p)] = t[p]
            for p in precisions[1:]:
                r["feature_max_over_range_" + p], r["feature_rms_over_range_" + p] = feature_distance(fes[p].features(wave)[1], hub)
        r["resample_ms"] = timed(lambda: audio.resample_poly(wave, 9, 8), args.repeat)
        r["mel_ms"] = timed(lambda: fe.mel(w18), args.repeat)
        if len(precisions) == 1:
            r["hubert_ms"] = timed(lambda: full.encode_long(wave), args.repeat)
        r["hubert_front_ms"] = timed(lambda: audio.chunked_encode(front.encode, norm), args.repeat)
        r["hubert_layers_ms"] = r["hubert_ms"] - r["hubert_front_ms"]
        for p in precisions[1:]:
            r["hubert_layers_ms_" + p] = r["hubert_ms_" + p] - r["hubert_front_ms"]
        out = torch.empty(N, 1024, device=dev)
        r["interp_ms"] = timed(lambda: audio._lib.check(audio._lib.lib().dsh_interp_time(audio._stream(torch.device(dev)), rows.data_ptr(), 1,
                                                                                         int(rows.shape[0]), 1024, out.data_ptr(), N)), args.repeat)
        with torch.no_grad():
            # chunk by chunk, as the reference runs it (one 20 s clip per forward)
            one = lambda enc: audio.chunked_encode(lambda b: torch.cat([enc(c[None]) for c in b]), norm)
            r["torch_oracle_fp32_ms"] = timed(lambda: one(lambda c: hubert_ref.encode(sd_dev, cfg_l, c, torch.float32, fast=True)), args.repeat)
            ref = one(lambda c: hubert_ref.encode(sd_dev, cfg_l, c, torch.float32, fast=True))
            r["max_abs_diff_vs_torch_fp32"] = float((ref - rows).abs().max())
            if hf is not None:
                r["transformers_fp32_ms"] = timed(lambda: one(lambda c: hf(c).last_hidden_state), args.repeat)
        r["sampling_ms"] = timed(lambda: tr.sample_arbitrary_len(mel[None], pid, {"pretrain_aud_feat": hub[None]}, seed=1), args.repeat)
        print(json.dumps(r))
        lines.append(r)
    if args.folder > 0:
        r = folder_case(fe, tr, cfg, args.folder, args.repeat, args.precision)
        if len(precisions) > 1:
            r.update(folder_precisions(fes, tr, cfg, args.folder, args.repeat))
            r["hubert_precisions"] = precisions
        print(json.dumps(r))
        lines.append(r)
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
