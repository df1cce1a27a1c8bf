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

Prints one JSON line per signal length (and one for the folder); --out also writes them to a file.

Usage:  python scripts/audio_frontend_bench.py [--seconds 60,600] [--folder 32] [--repeat 3] [--precision bf16] [--out FILE]
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "audio_frontend_bench needs a GPU"
    dev = "cuda:0"
    cfg_l = dict(hubert_ref.LARGE)
    sd = hubert_ref.make_state_dict(cfg_l, 1)
    full = audio.HubertEncoder(cfg_l, device=dev).load_state_dict(sd)
    front = audio.HubertEncoder(dict(cfg_l, layers=0), device=dev).load_state_dict({k: v for k, v in sd.items() if not k.startswith("encoder.layers.")})
    fe = audio.AudioFrontEnd(full)
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
        r = {"seconds": sec, "samples": n, "mel_frames": N, "hubert_rows": int(rows.shape[0]), "precision_sampler": args.precision}
        r["features_ms"] = timed(lambda: fe.features(wave), args.repeat)
        r["resample_ms"] = timed(lambda: audio.resample_poly(wave, 9, 8), args.repeat)
        r["mel_ms"] = timed(lambda: fe.mel(w18), args.repeat)
        r["hubert_ms"] = timed(lambda: full.encode_long(wave), args.repeat)
        r["hubert_front_ms"] = timed(lambda: audio.chunked_encode(front.encode, norm), args.repeat)
        r["hubert_layers_ms"] = r["hubert_ms"] - r["hubert_front_ms"]
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
        print(json.dumps(r))
        lines.append(r)
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
