#!/usr/bin/env python3
"""Motion-guidance fixtures: the imported reference (CPU) running its own ``ddim_sample_loop`` / ``p_sample_loop`` with a
``diffsheg_amd.glue.MotionGuidance(space="x_t")`` object as ``cond_fn`` (the object's plain-torch call IS the reference's hook:
condition_score / condition_mean, models/gaussian_diffusion.py:645-682).  Reuses make_golden.py's import recipe and helpers; same rules
(inputs are seeds, only expected outputs are stored).  The guidance terms are seeded too: tests/motion_guidance_ref.py, fixture_guidance().

  mguide_ddim25_plain_show.npz     ddim25_plain_show's inputs, attraction + velocity + acceleration terms
  mguide_harmonize_show_3_2.npz    ddim25_harmonize_show_3_2's inputs (masked window, RePaint schedule (3, 2)), attraction
  mguide_ddim25_eta05_show.npz     ddim25_eta05_show's inputs at eta = 0.5, attraction + velocity, a per-level scale ramp
  mguide_ddpm50_beat.npz           BEAT, ancestral loop on a 50-step linear schedule (the short-schedule trick of ddpm50_fhv_show),
                                   all three terms; also the unguided final sample of the same inputs (there is no such fixture)

Each holds the final sample, per-step corners and stats (the format tests/test_gpu_sampler.py's _check_trace reads) and
``moved``: max |guided - unguided| / max |unguided| of the final samples, which has to dwarf the parity tolerance.

Usage:  python tests/golden/make_golden_motion_guidance.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402
from make_golden import (SeededNoise, _masked_kwargs, _record_loop, build_ref_model, build_ref_samplers, get_config, make_inputs,  # noqa: E402
                         ref_opt, save)
from diffsheg_amd.glue import MotionGuidance  # noqa: E402
from motion_guidance_ref import fixture_guidance  # noqa: E402

MOVED_MIN = 0.05       # the guided final sample must differ from the unguided one by at least this fraction of its range (tolerance: 1e-3)


def guidance_for(case, B, T, C, diff):
    f = fixture_guidance(case, B, T, C, diff.num_timesteps)
    return MotionGuidance(f["target"], f["weight"], f["vel"], f["acc"], space="x_t", level_scale=f["level_scale"],
                          timestep_map=list(getattr(diff, "timestep_map", range(diff.num_timesteps))))


def _moved(final, base):
    m = float((final - base).abs().max() / base.abs().max())
    assert torch.isfinite(final).all() and m >= MOVED_MIN, f"guided sample moved by {m:.3g} of the range only (or is not finite)"
    return m


def _plain_kwargs(cfg, B, seed):
    inp = make_inputs(cfg, B, seed=seed)
    return {"audio_emb": inp["audio_emb"], "length": torch.full((B,), cfg.n_poses), "person_id": inp["person_id"],
            "add_cond": {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "y": {}, "pe_type": "pe_sinu"}


def gen_show(tr, gd, rs):
    cfg = get_config("show")
    opt = ref_opt(cfg)
    model, _ = build_ref_model(tr, cfg, opt)
    _, ddim = build_ref_samplers(gd, rs, opt)
    B = 2
    shape = (B, cfg.n_poses, cfg.net_dim_pose)
    dev = torch.device("cpu")
    # plain ddim25, all three terms
    src = SeededNoise(100)
    final, stats, corners = _record_loop(ddim.ddim_sample_loop_progressive(
        model, shape, clip_denoised=False, cond_fn=guidance_for("plain", *shape, ddim), model_kwargs=_plain_kwargs(cfg, B, 3), device=dev),
        src, "guided ddim25 plain")
    base = torch.from_numpy(np.load(os.path.join(HERE, "ddim25_plain_show.npz"))["final"])
    save("mguide_ddim25_plain_show.npz", batch=B, input_seed=3, noise_seed=100, draws=src.count, final=final, step_stats=stats,
         step_corner=corners, moved=_moved(final, base))
    # masked window on the (3, 2) RePaint schedule, attraction
    opt.jump_length, opt.jump_n_sample = 3, 2
    src = SeededNoise(101)
    final, stats, corners = _record_loop(ddim.ddim_sample_loop_progressive_harmonize(
        model, shape, clip_denoised=False, cond_fn=guidance_for("harmonize", *shape, ddim), model_kwargs=_masked_kwargs(cfg, B), device=dev),
        src, "guided harmonize (3,2)")
    opt.jump_length, opt.jump_n_sample = cfg.jump_length, cfg.jump_n_sample
    base = torch.from_numpy(np.load(os.path.join(HERE, "ddim25_harmonize_show_3_2.npz"))["final"])
    save("mguide_harmonize_show_3_2.npz", batch=B, input_seed=5, gt_seed=17, noise_seed=101, draws=src.count, final=final,
         step_stats=stats, step_corner=corners, moved=_moved(final, base))
    # eta = 0.5, attraction + velocity, per-level scales
    src = SeededNoise(100)
    final, stats, corners = _record_loop(ddim.ddim_sample_loop_progressive(
        model, shape, clip_denoised=False, cond_fn=guidance_for("eta", *shape, ddim), model_kwargs=_plain_kwargs(cfg, B, 3), device=dev,
        eta=0.5), src, "guided ddim25 eta=0.5")
    base = torch.from_numpy(np.load(os.path.join(HERE, "ddim25_eta05_show.npz"))["final"])
    save("mguide_ddim25_eta05_show.npz", batch=B, input_seed=3, noise_seed=100, eta=0.5, draws=src.count, final=final, step_stats=stats,
         step_corner=corners, moved=_moved(final, base))


def gen_beat_ddpm(tr, gd, rs, steps=50):
    cfg = get_config("beat")
    opt = ref_opt(cfg)
    model, _ = build_ref_model(tr, cfg, opt)
    g50 = gd.GaussianDiffusion(opt=opt, betas=gd.get_named_beta_schedule("linear", steps), model_mean_type=gd.ModelMeanType.EPSILON,
                               model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)
    B = 2
    shape = (B, cfg.n_poses, cfg.net_dim_pose)
    kw = _plain_kwargs(cfg, B, 3)
    src = SeededNoise(102)
    with mg.patched_noise(src), torch.no_grad():
        base = g50.p_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, device=torch.device("cpu"))
    src = SeededNoise(102)
    final, stats, corners = _record_loop(g50.p_sample_loop_progressive(
        model, shape, clip_denoised=False, cond_fn=guidance_for("ddpm", *shape, g50), model_kwargs=kw, device=torch.device("cpu")),
        src, f"guided ddpm{steps} beat")
    save(f"mguide_ddpm{steps}_beat.npz", batch=B, input_seed=3, noise_seed=102, diffusion_steps=steps, draws=src.count, final=final,
         final_unguided=base, step_stats=stats, step_corner=corners, moved=_moved(final, base))


def main():
    torch.manual_seed(0)
    tr, gd, rs, sch = mg.import_reference(with_trainer=False)
    gen_show(tr, gd, rs)
    gen_beat_ddpm(tr, gd, rs)


if __name__ == "__main__":
    main()
