#!/usr/bin/env python3
"""Two-sided (in-betweening / seam-repair) fixtures: the imported reference (CPU) runs its out-painting loop
``ddim_sample_loop_progressive_harmonize`` (models/gaussian_diffusion.py:1161-1278) on a mask that pins BOTH ends of a window,
``addBlend`` on, RePaint schedule (3, 5).  Reuses make_golden.py's helpers; same rules (inputs are seeds, only expected
outputs are stored).

  ddim25_twosided_show.npz   SHOW, B = 2, T = 88, L = 10: mask True on [:L] and [-L:]; gt[:, :L] (head) then gt[:, -L:] (tail)
                             drawn from one generator (gt seed 17), input seed 5, noise seed 101; recorded as gen_harmonize does
                             (final, per-step stats / corners of the denoise steps, draws)
  ddim25_twosided_beat.npz   the same for BEAT (T = 34, L = 4, no CFG)

Usage:  python tests/golden/make_golden_inbetween.py
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from make_golden import (SeededNoise, _record_loop, build_ref_model, build_ref_samplers, get_config, make_inputs, ref_opt,  # noqa: E402
                         save)


def twosided_kwargs(cfg, B, input_seed=5, gt_seed=17):
    """Conditioning of make_inputs(seed) + a gt / mask pair with the first and the last overlap_len frames pinned."""
    L = cfg.overlap_len
    inp = make_inputs(cfg, B, seed=input_seed)
    g = torch.Generator().manual_seed(gt_seed)
    gt = torch.zeros(B, cfg.n_poses, cfg.net_dim_pose)
    gt[:, :L] = torch.randn(B, L, cfg.net_dim_pose, generator=g)      # head first ...
    gt[:, -L:] = torch.randn(B, L, cfg.net_dim_pose, generator=g)     # ... then tail, same generator
    mask = torch.zeros_like(gt, dtype=torch.bool)
    mask[:, :L] = True
    mask[:, -L:] = True
    return {"audio_emb": inp["audio_emb"], "length": torch.full((B,), cfg.n_poses), "person_id": inp["person_id"],
            "add_cond": {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "y": {"gt": gt, "outpainting_mask": mask},
            "pe_type": "pe_sinu"}


def gen_twosided(tr, gd, rs, ds):
    cfg = get_config(ds)
    opt = ref_opt(cfg)
    assert opt.addBlend and (opt.jump_length, opt.jump_n_sample) == (3, 5)
    model, _ = build_ref_model(tr, cfg, opt)
    _, ddim = build_ref_samplers(gd, rs, opt)
    B, L = 2, cfg.overlap_len
    kw = twosided_kwargs(cfg, B)
    src = SeededNoise(101)
    final, stats, corners = _record_loop(
        ddim.ddim_sample_loop_progressive_harmonize(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False,
                                                    model_kwargs=kw, device=torch.device("cpu")), src, f"two-sided {ds}")
    gt = kw["y"]["gt"]
    # the pinned tail carries no fade in the reference (addBlend touches the first L frames only); head frame 0 has weight 0
    assert torch.allclose(final[:, -L:], gt[:, -L:], atol=1e-5) and torch.allclose(final[:, 0], gt[:, 0], atol=1e-5)
    save(f"ddim25_twosided_{ds}.npz", batch=B, input_seed=5, gt_seed=17, noise_seed=101, overlap_len=L,
         draws=src.count, final=final, step_stats=stats, step_corner=corners)


def main():
    torch.set_num_threads(8)
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="show,beat")
    only = set(ap.parse_args().only.split(","))
    tr, gd, rs, _ = mg.import_reference(with_trainer=False)
    for ds in ("show", "beat"):
        if ds in only:
            print(f"two-sided {ds}"); gen_twosided(tr, gd, rs, ds)


if __name__ == "__main__":
    main()
