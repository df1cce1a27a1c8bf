#!/usr/bin/env python3
"""Evaluations of one padded batch with and without per-clip lengths, for a kernel trace: run it under
``rocprofv3 --kernel-trace --stats -d DIR -o p -- python scripts/ragged_attention_profile.py`` and read the attention kernels' rows of
``scripts/rocprof_summary.py DIR/.../p_results.db`` — ``linear_attention_*<false>`` is the full-length launch, ``<true>`` the ragged one.

usage: python scripts/ragged_attention_profile.py [--batch 950] [--precision bf16] [--dataset show] [--evals 5]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.model import UniDiffuser  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from diffsheg_amd.weights import make_synthetic_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=950)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--dataset", default="show", choices=["show", "beat"])
    ap.add_argument("--evals", type=int, default=5)
    args = ap.parse_args()
    cfg = get_config(args.dataset)
    model = UniDiffuser(cfg, make_synthetic_state_dict(cfg, 1234), device="cuda:0", precision=args.precision)
    B, T = args.batch, cfg.n_poses
    small = make_inputs(cfg, min(B, 64), seed=3)
    rep = (B + 63) // 64
    x, a, h = (small[k].repeat(rep, 1, 1)[:B].cuda().contiguous() for k in ("x_T", "audio_emb", "pretrain_aud_feat"))
    pid = torch.zeros(B, cfg.style_dim, device="cuda:0")
    pid[torch.arange(B), torch.arange(B) % cfg.style_dim] = 1.0
    t = torch.full((B,), 520, dtype=torch.long, device="cuda:0")
    sa = [torch.full((B, 1, 1), 1.7, device="cuda:0"), torch.full((B, 1, 1), 1.3, device="cuda:0")]
    pat = [T, (7 * T) // 10, (2 * T) // 9, 4, T - 1, 33, 32, 12, 1, 24, (T + 1) // 2]
    lens = torch.tensor([min(T, pat[b % len(pat)]) for b in range(B)])
    for length in (None, lens):
        for _ in range(args.evals):
            out = model(x, t, sqrt_alphas=sa, audio_emb=a, length=length, person_id=pid, add_cond={"pretrain_aud_feat": h}, y={})
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
    print(f"{args.dataset} {args.precision} B={B} T={T}: {args.evals} evaluations without lengths, {args.evals} with lengths of mean {float(lens.float().mean()):.1f} frames")


if __name__ == "__main__":
    main()
