#!/usr/bin/env python3
"""Kernel times of the HuBERT encoder's bf16 precision mode, per layer shape on random operands:

  new      dsh_op_gemm_bf16_pro in the form the encoder launches it (LayerNorm shapes: fp32 A with row moments passed in, bf16 store, GELU for
           intermediate_dense; the two residual shapes: bf16 A, fp32 residual in place), both tile shapes, and the row-moments launch alone
           (mom = None makes the op compute them: that call is timed too and includes a scratch allocation, so only the difference of the
           kernel times in a rocprofv3 trace is the launch's cost);
  bf16_nt  the existing gemm_nt_kernel<bf16> (dsh_op_gemm, dtype 1) on a bf16 A that is already normalised: the baseline WITHOUT the
           launch_ln_rows<bf16> pass it needs in front of the two LayerNorm shapes (a lower bound of the baseline);
  f32_pro  gemm_f32_pro (pro 0) on fp32 operands, what the fp32 encoder runs;
and dsh_op_softmax_attention_bf16 against dsh_op_softmax_attention at M = 1000.

Times are event-timed medians; run the script under `rocprofv3 --kernel-trace --stats -- python scripts/hubert_bf16_kernels_bench.py --shape K,N`
(one shape per process, no counters in the same run) for the per-kernel figures.  Prints one JSON line per case.

Usage:  python scripts/hubert_bf16_kernels_bench.py [--rows 8000] [--repeat 5] [--shape 1024,3072] [--attention]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffsheg_amd import _lib  # noqa: E402

LAYER_SHAPES = [(1024, 3072), (1024, 1024), (1024, 4096), (4096, 1024)]      # q|k|v, out_proj, intermediate_dense, output_dense


def timed(fn, repeat: int) -> float:
    """median time of fn() in ms by stream events, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--shape", default=None, help="K,N: one layer shape instead of all four")
    ap.add_argument("--attention", action="store_true", help="the attention kernels only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hubert_bf16_kernels_bench needs a GPU"
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(1)
    R = args.rows
    shapes = [tuple(int(v) for v in args.shape.split(","))] if args.shape else ([] if args.attention else LAYER_SHAPES)
    for K, N in shapes:
        ln = (K, N) in ((1024, 3072), (1024, 4096))            # the two shapes with a LayerNorm in front
        x32 = torch.randn(R, K, generator=g).cuda()
        x16 = x32.bfloat16()
        w32 = (torch.randn(N, K, generator=g) / K ** 0.5).cuda()
        w16 = w32.bfloat16()
        bias = torch.randn(N, generator=g).cuda()
        mom = torch.stack((x32.mean(1), 1 / torch.sqrt(x32.var(1, unbiased=False) + 1e-5)), 1).contiguous()
        of, ob = torch.zeros(R, N, device="cuda"), torch.zeros(R, N, device="cuda", dtype=torch.bfloat16)
        flop = 2.0 * R * K * N
        r = {"K": K, "N": N, "rows": R, "layernorm_shape": ln}

        def new(tile, m=mom):
            if ln:
                return L.dsh_op_gemm_bf16_pro(st, x32.data_ptr(), 1, m.data_ptr() if m is not None else None, w16.data_ptr(), bias.data_ptr(), None, None,
                                              ob.data_ptr(), R, N, K, 2 if N == 4096 else 0, tile)
            return L.dsh_op_gemm_bf16_pro(st, x16.data_ptr(), 0, None, w16.data_ptr(), bias.data_ptr(), of.data_ptr(), of.data_ptr(), None, R, N, K, 0, tile)

        def nt():
            if ln:
                return L.dsh_op_gemm(st, 1, x16.data_ptr(), w16.data_ptr(), bias.data_ptr(), None, None, ob.data_ptr(), R, N, K, 2 if N == 4096 else 0)
            return L.dsh_op_gemm(st, 1, x16.data_ptr(), w16.data_ptr(), bias.data_ptr(), of.data_ptr(), of.data_ptr(), None, R, N, K, 0)

        def f32():
            z = None
            return L.dsh_op_gemm_f32_pro(st, 0, x32.data_ptr(), K, K, z, 0, 0, z, 0, 0, z, 0, 0, K, w32.data_ptr(), bias.data_ptr(), z, z, 0, 0, 0, 0,
                                         None if ln else of.data_ptr(), of.data_ptr(), R, N, 2 if N == 4096 else 0, z, 0, z)

        for name, fn in (("new_tile64", lambda: new(1)), ("new_tile128", lambda: new(2)), ("bf16_nt", nt), ("f32_pro", f32)):
            assert fn() == 0, (name, L.dsh_last_error())
            ms = timed(fn, args.repeat)
            r[name + "_ms"], r[name + "_tflops"] = ms, flop / ms * 1e-9
        if ln:
            r["new_with_own_moments_ms"] = timed(lambda: new(0, None), args.repeat)
        print(json.dumps(r))
    if args.attention or not args.shape:
        B, M, H = 8, 1000, 16
        q32 = torch.randn(B, M, 3 * H * 64, generator=g).cuda()
        q32[:, :, :H * 64] *= 0.125
        q16 = q32.bfloat16()
        o32, o16 = torch.zeros(B, M, H * 64, device="cuda"), torch.zeros(B, M, H * 64, device="cuda", dtype=torch.bfloat16)
        flop = 4.0 * B * H * M * M * 64
        t16 = timed(lambda: L.dsh_op_softmax_attention_bf16(st, q16.data_ptr(), B, M, H, o16.data_ptr()), args.repeat)
        t32 = timed(lambda: L.dsh_op_softmax_attention(st, q32.data_ptr(), B, M, H, o32.data_ptr()), args.repeat)
        print(json.dumps({"attention": [B, M, H], "bf16_ms": t16, "bf16_tflops": flop / t16 * 1e-9, "f32_ms": t32, "f32_tflops": flop / t32 * 1e-9,
                          "max_abs_diff": float((o16.float() - o32).abs().max())}))


if __name__ == "__main__":
    main()
