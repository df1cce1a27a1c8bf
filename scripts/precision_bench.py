#!/usr/bin/env python3
"""precision="fp32" against precision="bf16x3" (DESIGN.md §4.21): the same model on the exact-fp32 MFMA and on the split-bf16 main loop
(three bf16 MFMAs per product, gemm_f32_split.hip), in ONE process, timed ALTERNATELY (round r of both before round r + 1 of either), so
that clock and pool drift hit both alike.

  (a) per launch, the four Linear shapes of the §4.7 table at M = 8704 token rows through dsh_op_gemm_f32_pro_ex (mma 0 / 1, and the split
      loop's two tile shapes): q|k|v with its folded LayerNorm (pro 1), the StylizationBlock Linear (pro 2), feat_proj.1 over the padded concat
      (pro 1, K = 960) and feat_proj.3 (pro 0, K = 1024, residual in place).  Every timed call takes the next of --sets operand sets (rows,
      weights, output), so that a launch does not find its own operands of the previous call in the caches.  The weights of the split
      launches are packed once per operand set (dsh_op_split_pack_weight, as the model packs at finalisation) and passed packed (mma + 64):
      every timed call is one launch, device events around a burst of them;
  (b) one evaluation and one ddim25 generate_batch at BEAT B = 256 and SHOW B = 950 (CFG 1.25), wall time around a device synchronise;
  (c) max and rms |sample(bf16x3) - sample(fp32)| of the ddim25 results at the same seed, as a share of the fp32 sample's range.

Prints one JSON line per measurement; --out also writes them to a file.  Needs a GPU: there is no CPU fallback.

Usage:  python scripts/precision_bench.py [--repeat 5] [--sets 4] [--m 8704] [--skip-model] [--batches beat:256,show:950] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffsheg_amd import _lib  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.model import UniDiffuser  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from diffsheg_amd.weights import make_synthetic_state_dict  # noqa: E402

P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
DEV = "cuda:0"
PRECISIONS = ("fp32", "bf16x3")
FP32_MFMA_PEAK_TF = 157.3


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


# ---- (a) the Linear shapes ------------------------------------------------------------------------------------------------------------------
def linear_shapes(M, sets, g):
    """name -> (N, K, [call(mma) per operand set])"""
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    L = _lib.lib()
    shapes = {}

    def both(W):
        """mma -> the weight operand of that loop: fp32 as it is, or packed once for the split loop"""
        Wp = torch.empty(W.shape, dtype=torch.int32, device=DEV)
        _lib.check(L.dsh_op_split_pack_weight(None, P(W), W.shape[0], W.shape[1], P(Wp)))
        return lambda mma: P(W) if mma == 0 else P(Wp)

    def qkv():
        x, W, b, fc, out = rn(M, 512), rn(1536, 512) / 23, rn(1536), rn(1536), torch.empty(M, 1536, device=DEV)
        Wm = both(W)
        return lambda mma: L.dsh_op_gemm_f32_pro_ex(None, 1, P(x), 512, 512, None, 0, 0, None, 0, 0, None, 0, 0, 512, Wm(mma), P(b), P(fc), None, 0, 0, 1, 1, None, P(out),
                                                    M, 1536, 0, None, 0, None, mma)

    def sty():
        nb = max(1, M // 34)
        x, film, W, b, h = rn(M, 512), rn(nb, 1024), rn(512, 512) / 23, rn(512), rn(M, 512)
        Wm = both(W)
        return lambda mma: L.dsh_op_gemm_f32_pro_ex(None, 2, P(x), 512, 512, None, 0, 0, None, 0, 0, None, 0, 0, 512, Wm(mma), P(b), None, P(film), 1024, 0, 34, nb, P(h), P(h),
                                                    M, 512, 0, None, 0, None, mma)

    def feat1():
        s0, s1, s2, s3 = rn(M, 512), rn(M, 256), rn(M, 128), rn(M, 64)
        s3[:, 51:] = 0
        W, b, fc, out = rn(1024, 960) / 31, rn(1024), rn(1024), torch.empty(M, 1024, device=DEV)
        W[:, 947:] = 0
        Wm = both(W)
        return lambda mma: L.dsh_op_gemm_f32_pro_ex(None, 1, P(s0), 512, 512, P(s1), 256, 256, P(s2), 128, 128, P(s3), 64, 64, 947, Wm(mma), P(b), P(fc), None, 0, 0, 1, 1, None,
                                                    P(out), M, 1024, 1, None, 0, None, mma)

    def feat3():
        A, W, b, R = rn(M, 1024), rn(512, 1024) / 32, rn(512), rn(M, 512)
        Wm = both(W)
        return lambda mma: L.dsh_op_gemm_f32_pro_ex(None, 0, P(A), 1024, 1024, None, 0, 0, None, 0, 0, None, 0, 0, 1024, Wm(mma), P(b), None, None, 0, 0, 1, 1, P(R), P(R),
                                                    M, 512, 0, None, 0, None, mma)

    for name, N, K, make in (("q|k|v (pro 1)", 1536, 512, qkv), ("StylizationBlock (pro 2)", 512, 512, sty), ("feat_proj.1 (pro 1, concat)", 1024, 960, feat1),
                             ("feat_proj.3 (pro 0)", 512, 1024, feat3)):
        shapes[name] = (N, K, [make() for _ in range(sets)])
    return shapes


def time_linears(M, sets, repeat, emit):
    g = torch.Generator(device=DEV).manual_seed(1)
    n_call = max(20, 4 * sets)
    for name, (N, K, calls) in linear_shapes(M, sets, g).items():
        def burst(mma):
            """us per call over n_call calls cycling the operand sets, device events around the burst"""
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(n_call):
                _lib.check(calls[i % sets](mma))
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / n_call
        modes = {"fp32": 0, "bf16x3": 1 + 64, "bf16x3_tile64": 1 + 16 + 64, "bf16x3_tile128": 1 + 32 + 64}
        for m in modes.values():
            burst(m)                                                # warm-up of every kernel the window uses
        us = {k: [] for k in modes}
        for _ in range(repeat):
            for k, m in modes.items():
                us[k].append(burst(m))
        med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
        fl = 2.0 * M * N * K
        emit({"what": "linear", "name": name, "M": M, "N": N, "K": K, "operand_sets": sets, "us_fp32": round(med["fp32"], 1),
              "us_bf16x3": round(med["bf16x3"], 1), "us_bf16x3_tile64": round(med["bf16x3_tile64"], 1),
              "us_bf16x3_tile128": round(med["bf16x3_tile128"], 1),
              "tf_fp32": round(fl / med["fp32"] / 1e6, 1), "share_of_fp32_mfma_peak_fp32": round(fl / med["fp32"] / 1e6 / FP32_MFMA_PEAK_TF, 3),
              "tf_bf16x3": round(fl / med["bf16x3"] / 1e6, 1), "ratio_fp32_over_bf16x3": round(med["fp32"] / med["bf16x3"], 2)})


# ---- (b), (c) the models ----------------------------------------------------------------------------------------------------------------------
def time_models(ds, B, repeat, emit):
    cfg = get_config(ds)
    sd = make_synthetic_state_dict(cfg, 1234)
    inp = make_inputs(cfg, B, seed=3)
    T = inp["x_T"].shape[1]
    a, p, cnd = inp["audio_emb"].to(DEV), inp["person_id"].to(DEV), {"pretrain_aud_feat": inp["pretrain_aud_feat"].to(DEV)}
    x, t = inp["x_T"].to(DEV), torch.full((B,), 420, dtype=torch.long, device=DEV)
    shape_e = (B, T, cfg.expression_dim)
    sa = [torch.full(shape_e, 1.3), torch.full(shape_e, 0.8)]
    models = {prec: UniDiffuser(cfg, sd, device=DEV, precision=prec) for prec in PRECISIONS}
    trainers = {prec: DDPMTrainer(sampler_namespace(cfg), m) for prec, m in models.items()}
    keep = {}

    def evaluation(prec):
        def f():
            keep["eps_" + prec] = models[prec](x, t, sqrt_alphas=sa, audio_emb=a, length=torch.full((B,), T), person_id=p, add_cond=cnd, pe_type="pe_sinu", y={})
        return f

    def loop(prec):
        def f():
            keep["x_" + prec] = trainers[prec].generate_batch(a, p, cfg.net_dim_pose, cnd, {}, seed=2024)
        return f

    ev = timed_alternately({prec: evaluation(prec) for prec in PRECISIONS}, repeat)
    _lib.launch_counts(reset=True)
    evaluation("bf16x3")()
    torch.cuda.synchronize()
    counts = _lib.launch_counts(reset=True)
    lp = timed_alternately({prec: loop(prec) for prec in PRECISIONS}, repeat)
    row = {"what": "model", "dataset": ds, "B": B, "T": T, "cfg": f"cond_scale={cfg.cond_scale}" if cfg.cfg_active else "no CFG", "repeat": repeat,
           "split_launches_per_eval": counts["gemm_f32_split"], "exact_fp32_pro_launches_per_eval": counts["gemm_f32_pro"]}
    for prec in PRECISIONS:
        row[f"eval_ms_{prec}"] = round(ev[prec], 2)
        row[f"ddim25_ms_{prec}"] = round(lp[prec], 1)
        row[f"ddim25_kframes_per_s_{prec}"] = round(B * T / lp[prec], 1)
    row["eval_ratio_fp32_over_bf16x3"] = round(ev["fp32"] / ev["bf16x3"], 3)
    row["ddim25_ratio_fp32_over_bf16x3"] = round(lp["fp32"] / lp["bf16x3"], 3)
    for key, what in (("eps", "eval"), ("x", "ddim25")):
        ref, got = keep[f"{key}_fp32"].double(), keep[f"{key}_bf16x3"].double()
        rng = float(ref.max() - ref.min())
        d = got - ref
        row[f"{what}_max_diff_of_range"] = float(d.abs().max()) / rng
        row[f"{what}_rms_diff_of_range"] = float(d.pow(2).mean().sqrt()) / rng
    emit(row)
    del models, trainers
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--sets", type=int, default=4, help="operand sets a per-launch window cycles through")
    ap.add_argument("--m", type=int, default=8704)
    ap.add_argument("--batches", default="beat:256,show:950")
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-linears", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("precision_bench.py needs a GPU: there is no CPU fallback")
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if not args.skip_linears:
        time_linears(args.m, args.sets, args.repeat, emit)
    if not args.skip_model:
        for item in args.batches.split(","):
            ds, B = item.split(":")
            time_models(ds, int(B), args.repeat, emit)


if __name__ == "__main__":
    main()
