#!/usr/bin/env python3
"""Fixtures for few-step sampling, from the imported reference on the CPU (development container only, like make_golden.py):

  fewstep_tables.npz       the reference SpacedDiffusion's fp64 tables and timestep_map for space_timesteps(1000, "10"), "4,3,3", ddim10
                           and the logsnr8 set
  fewstep_plain_beat.npz   BEAT, B = 2, recorded noise: the reference's own ddim_sample_loop on the logsnr8 set (per-step corners as in
                           ddim25_plain_*), and the dpm2m loop of tests/fewstep_ref.py driven by the reference model as eps function on
                           the same inputs — plain, and one masked window with its explicit schedule

Usage:  python tests/golden/make_golden_fewstep.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402
import fewstep_ref as F  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.synthetic import SeededNoise, make_inputs  # noqa: E402

NAMES = ["betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
         "posterior_variance", "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2"]


def spaced(gd, rs, opt, use):
    betas = gd.get_named_beta_schedule("linear", 1000)
    return rs.SpacedDiffusion(use_timesteps=use, rescale_timesteps=False, opt=opt, betas=betas, model_mean_type=gd.ModelMeanType.EPSILON,
                              model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)


def gen_tables(gd, rs):
    opt = G.ref_opt(get_config("show"))
    out = {}
    for tag, use in (("s10", rs.space_timesteps(1000, "10")), ("s433", rs.space_timesteps(1000, "4,3,3")),
                     ("ddim10", rs.space_timesteps(1000, "ddim10")), ("logsnr8", set(F.LOGSNR8))):
        d = spaced(gd, rs, opt, use)
        out[f"{tag}__timestep_map"] = np.array(d.timestep_map)
        for n in NAMES:
            out[f"{tag}__{n}"] = getattr(d, n)
    G.save("fewstep_tables.npz", **out)


class _Recorded:
    """oracle NoiseSource interface over a SeededNoise (same draws as the native loop's noise_source)."""

    def __init__(self, seed):
        self.src = SeededNoise(seed)

    def randn(self, shape):
        return self.src.randn(tuple(shape))


def gen_plain_beat(tr, gd, rs):
    cfg = get_config("beat")
    opt = G.ref_opt(cfg)
    model, _ = G.build_ref_model(tr, cfg, opt)
    B, T, C = 2, cfg.n_poses, cfg.net_dim_pose
    inp = make_inputs(cfg, B, seed=3)
    kw = {"audio_emb": inp["audio_emb"], "length": torch.full((B,), T), "person_id": inp["person_id"],
          "add_cond": {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "y": {}, "pe_type": "pe_sinu"}
    out = {"batch": B, "input_seed": 3, "noise_seed": 100, "kept": np.array(F.LOGSNR8)}
    # (a) the reference's own loop on the logsnr8 set
    d = spaced(gd, rs, opt, set(F.LOGSNR8))
    src = SeededNoise(100)
    final, stats, corners = G._record_loop(
        d.ddim_sample_loop_progressive(model, (B, T, C), clip_denoised=False, model_kwargs=kw, device=torch.device("cpu")), src, "logsnr8 ddim beat")
    out.update(ddim_draws=src.count, ddim_final=final, ddim_step_stats=stats, ddim_step_corner=corners)

    # (b) the dpm2m loop of fewstep_ref with the reference model as eps function
    shape_e = (B, T, cfg.expression_dim)

    def eps_fn(x, t_orig, c1, c2):
        with torch.no_grad():
            return model(x, torch.full((B,), int(t_orig), dtype=torch.long), [torch.full(shape_e, float(c1)), torch.full(shape_e, float(c2))],
                         inp["audio_emb"], torch.full((B,), T, dtype=torch.long), inp["person_id"],
                         {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "pe_sinu", {})

    def record(trace):
        den = [t for t in trace if t[0] == "denoise"]
        st = [G.step_stats(t[2]) for t in den]
        return np.stack([s[0] for s in st]), np.stack([s[1] for s in st])

    ns, trace = _Recorded(100), []
    final = F.sample_loop(eps_fn, (B, T, C), {}, ns, F.LOGSNR8, solver="dpm2m", overlap_len=cfg.overlap_len, trace=trace)
    stats, corners = record(trace)
    out.update(dpm_draws=ns.src.count, dpm_final=final, dpm_step_stats=stats, dpm_step_corner=corners)
    print(f"  logsnr8 dpm2m beat: draws={ns.src.count}, |x|max={final.abs().max():.3g}")

    # (c) one masked window: gt / mask as the ddim25_harmonize fixtures build them, schedule walked from the subset's own start level
    mk = G._masked_kwargs(cfg, B)
    inp = make_inputs(cfg, B, seed=5)
    t_T = F.masked_start_level(1000, F.LOGSNR8)
    times = F.jump_schedule_from(t_T, cfg.jump_length, cfg.jump_n_sample)
    ns, trace = _Recorded(101), []
    final = F.sample_loop(eps_fn, (B, T, C), mk["y"], ns, F.LOGSNR8, solver="dpm2m", times=times, overlap_len=cfg.overlap_len,
                          add_blend=cfg.add_blend, trace=trace)
    stats, corners = record(trace)
    out.update(masked_input_seed=5, masked_gt_seed=17, masked_noise_seed=101, masked_t_T=t_T, masked_times=np.array(times),
               masked_draws=ns.src.count, masked_final=final, masked_step_stats=stats, masked_step_corner=corners)
    print(f"  logsnr8 dpm2m masked beat: t_T={t_T}, {len(times) - 1} steps, draws={ns.src.count}, |x|max={final.abs().max():.3g}")
    G.save("fewstep_plain_beat.npz", **out)


if __name__ == "__main__":
    tr, gd, rs, sch = G.import_reference(with_trainer=False)
    gen_tables(gd, rs)
    gen_plain_beat(tr, gd, rs)
