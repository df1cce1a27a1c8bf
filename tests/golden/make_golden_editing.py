#!/usr/bin/env python3
"""Editing fixtures: the imported reference (CPU) restarts its DDIM loop from a level, re-samples a region of an existing motion and
runs its reverse ODE.  Reuses make_golden.py's helpers; same rules (inputs are seeds, only expected outputs are stored).  Every loop
here is the reference's own per-step function (``q_sample`` models/gaussian_diffusion.py:417-462, ``ddim_sample`` :976-1066, ``undo``
:464-473, ``ddim_reverse_sample`` :1068-1104) called level by level on the ddim25 ``SpacedDiffusion``, B = 2, K = 10, fp32,
``clip_denoised=False``; x0 ~ N(0, 1) from ``torch.Generator().manual_seed(x0_seed)``, conditioning ``make_inputs(seed 3)``.

  edit_restart_{show,beat}.npz  x = q_sample(x0, 9, noise = draw 0), then ddim_sample at levels 9 .. 0 under patched_noise(SeededNoise):
                                final, per-step stats / corners (10 rows), draws (11)
  edit_keep_show.npz            the same with gt = x0 and keep = frames [:20] plus columns [0, 30) everywhere, addBlend off, walking the
                                RePaint jump schedule from t_T = 10 at (3, 5): ddim_sample for a downward pair, undo for an upward
                                one; one stats / corner row per PAIR (undo steps included, the order of a native trace)
  edit_invert_{show,beat}.npz   ddim_reverse_sample at levels 0 .. 9 from x0: final, per-step stats / corners; no draws
  edit_tables_ddim25.npz        alphas_cumprod_next of the ddim25 SpacedDiffusion, float64

Usage:  python tests/golden/make_golden_editing.py [--only restart,keep,invert,tables]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from make_golden import (SeededNoise, build_ref_model, build_ref_samplers, get_config, make_inputs, patched_noise, ref_opt,  # noqa: E402
                         save, step_stats)

K, B, X0_SEED, INPUT_SEED, NOISE_SEED = 10, 2, 41, 3, 103
KEEP_FRAMES, KEEP_COLS = 20, 30


def walk_from(t_T: int, jump_length: int, jump_n_sample: int):
    """The RePaint time list walked from ``t_T``: down one level at a time; the first ``jump_n_sample - 1`` times a level
    ``0, jump_length, 2 jump_length, .. < t_T - jump_length`` is reached, ``jump_length`` levels back up.  Ends with -1.  At the
    reference's built-in ``t_T`` this is its ``get_schedule_jump_cjm_ddim`` (checked in :func:`gen_keep`)."""
    left = {j: jump_n_sample - 1 for j in range(0, t_T - jump_length, jump_length)}
    t, ts = t_T, []
    while t >= 1:
        t -= 1
        ts.append(t)
        if left.get(t, 0) > 0:
            left[t] -= 1
            for _ in range(jump_length):
                t += 1
                ts.append(t)
    return ts + [-1]


def _setup(tr, gd, rs, ds, **opt_over):
    cfg = get_config(ds)
    opt = ref_opt(cfg)
    for k, v in opt_over.items():
        setattr(opt, k, v)
    model, _ = build_ref_model(tr, cfg, opt)
    _, ddim = build_ref_samplers(gd, rs, opt)
    inp = make_inputs(cfg, B, seed=INPUT_SEED)
    x0 = torch.randn(B, cfg.n_poses, cfg.net_dim_pose, generator=torch.Generator().manual_seed(X0_SEED))
    kw = {"audio_emb": inp["audio_emb"], "length": torch.full((B,), cfg.n_poses), "person_id": inp["person_id"],
          "add_cond": {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "y": {}, "pe_type": "pe_sinu"}
    return cfg, opt, model, ddim, x0, kw


def _t(k):
    return torch.full((B,), k, dtype=torch.long)


def gen_restart(tr, gd, rs, ds):
    cfg, opt, model, ddim, x0, kw = _setup(tr, gd, rs, ds)
    src = SeededNoise(NOISE_SEED)
    stats, corners = [], []
    t0 = time.time()
    with patched_noise(src), torch.no_grad():
        x = ddim.q_sample(x0, _t(K - 1), noise=src.randn(tuple(x0.shape)))
        for k in range(K - 1, -1, -1):
            x = ddim.ddim_sample(model, x, _t(k), clip_denoised=False, model_kwargs=kw)["sample"]
            s, c = step_stats(x)
            stats.append(s); corners.append(c)
    print(f"  restart {ds}: {time.time()-t0:.1f}s, draws={src.count}, |x|max={x.abs().max():.3g}")
    assert src.count == K + 1
    save(f"edit_restart_{ds}.npz", batch=B, level=K, x0_seed=X0_SEED, input_seed=INPUT_SEED, noise_seed=NOISE_SEED, draws=src.count,
         final=x, step_stats=np.stack(stats), step_corner=np.stack(corners))


def gen_keep(tr, gd, rs, sch, ds="show"):
    cfg, opt, model, ddim, x0, kw = _setup(tr, gd, rs, ds, addBlend=False)
    assert (opt.jump_length, opt.jump_n_sample) == (3, 5)
    assert walk_from(15, 3, 5) == list(sch.get_schedule_jump_cjm_ddim(25, jump_length=3, jump_n_sample=5))
    assert walk_from(15, 1, 1) == list(sch.get_schedule_jump_cjm_ddim(25))
    keep = torch.zeros(B, cfg.n_poses, cfg.net_dim_pose, dtype=torch.bool)
    keep[:, :KEEP_FRAMES] = True
    keep[:, :, :KEEP_COLS] = True
    kw["y"] = {"gt": x0.clone(), "outpainting_mask": keep}
    times = walk_from(K, 3, 5)
    src = SeededNoise(NOISE_SEED)
    stats, corners = [], []
    t0 = time.time()
    with patched_noise(src), torch.no_grad():
        x = ddim.q_sample(x0, _t(K - 1), noise=src.randn(tuple(x0.shape)))
        for t_last, t_cur in zip(times[:-1], times[1:]):
            if t_cur < t_last:
                out = ddim.ddim_sample(model, x, _t(t_last), clip_denoised=False, model_kwargs=kw)
                x = out["sample"]
            else:
                x = ddim.undo(x, x, est_x_0=out["pred_xstart"], t=_t(t_last))
            s, c = step_stats(x)
            stats.append(s); corners.append(c)
    print(f"  keep {ds}: {time.time()-t0:.1f}s, {len(stats)} steps, draws={src.count}, |x|max={x.abs().max():.3g}")
    assert torch.equal(x[keep], x0[keep])
    save(f"edit_keep_{ds}.npz", batch=B, level=K, x0_seed=X0_SEED, input_seed=INPUT_SEED, noise_seed=NOISE_SEED, draws=src.count,
         keep_frames=KEEP_FRAMES, keep_cols=KEEP_COLS, steps=len(stats), final=x, step_stats=np.stack(stats),
         step_corner=np.stack(corners))


def gen_invert(tr, gd, rs, ds):
    cfg, opt, model, ddim, x0, kw = _setup(tr, gd, rs, ds)
    stats, corners = [], []
    t0 = time.time()
    x = x0
    with torch.no_grad():
        for k in range(K):
            x = ddim.ddim_reverse_sample(model, x, _t(k), clip_denoised=False, model_kwargs=kw)["sample"]
            s, c = step_stats(x)
            stats.append(s); corners.append(c)
    print(f"  invert {ds}: {time.time()-t0:.1f}s, |x|max={x.abs().max():.3g}")
    save(f"edit_invert_{ds}.npz", batch=B, level=K, x0_seed=X0_SEED, input_seed=INPUT_SEED, final=x, step_stats=np.stack(stats),
         step_corner=np.stack(corners))


def gen_tables(gd, rs):
    _, ddim = build_ref_samplers(gd, rs, ref_opt(get_config("show")))
    save("edit_tables_ddim25.npz", alphas_cumprod_next=np.asarray(ddim.alphas_cumprod_next, dtype=np.float64))


def main():
    torch.set_num_threads(8)
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="restart,keep,invert,tables")
    only = set(ap.parse_args().only.split(","))
    tr, gd, rs, sch = mg.import_reference(with_trainer=False)
    if "tables" in only:
        gen_tables(gd, rs)
    for ds in ("show", "beat"):
        if "restart" in only:
            gen_restart(tr, gd, rs, ds)
        if "invert" in only:
            gen_invert(tr, gd, rs, ds)
    if "keep" in only:
        gen_keep(tr, gd, rs, sch)


if __name__ == "__main__":
    main()
