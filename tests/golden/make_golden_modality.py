#!/usr/bin/env python3
"""One-modality fixtures: gestures for a GIVEN expression track, from the imported reference (CPU).  Reuses make_golden.py's helpers;
same rules (inputs are seeds, only expected outputs are stored).

The reference wires its gesture encoder to the expression encoder's x0 estimate inside ``UniDiffuser.forward`` (models/transformer.py:
730-763).  ``GivenTrack`` below calls the REAL module's ``time_embed``, ``encoder_aud`` and ``encoder_ges`` exactly as those lines do,
with ``expr_cond`` (:749) replaced by a seeded given track; ``encoder_exp`` is not called and the expression columns of its output are 0.
The reference's own sampling loops then drive it at full width (full-width noise draws): the gesture columns of their results are
what is stored — every sampler update is element-wise, so they do not depend on what the expression columns do.

  modality_show.npz   SHOW, B = 2, T = 88: eps_ges at ddim25 levels k0 / k14, a plain ddim25 loop, one out-painting window (3, 5)
  modality_beat.npz   BEAT, B = 3, T = 34: the same

Usage:  python tests/golden/make_golden_modality.py
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from make_golden import (SeededNoise, _masked_kwargs, _record_loop, build_ref_model, build_ref_samplers, get_config, make_inputs,  # noqa: E402
                         ref_opt, save)

TRACK_SEED, EVAL_SEED, LOOP_NOISE, MASKED_NOISE = 77, 3, 100, 101
BATCH = {"show": 2, "beat": 3}


def make_track(cfg, B, seed=TRACK_SEED):
    """The given expression track [B, T, E]: standardised values ~ N(0, 1) from a seeded CPU generator."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, cfg.n_poses, cfg.expression_dim, generator=g)


class GivenTrack:
    """transformer.py:730-763 on the real sub-modules, with expr_cond = the given track."""

    def __init__(self, tr, model, track):
        self.tr, self.m, self.track = tr, model, track

    def parameters(self):
        return self.m.parameters()

    def __call__(self, x, timesteps, sqrt_alphas, audio_emb, length, person_id, add_cond={}, pe_type="learnable", y=None):
        m = self.m
        emb = m.time_embed(self.tr.timestep_embedding(timesteps, m.latent_dim))
        T = x.shape[1]
        src_mask = m.generate_src_mask(T, length).to(x.device).unsqueeze(-1)
        audio_feat = m.encoder_aud(audio_emb, None, emb, src_mask, {})
        audio_emb = torch.cat((audio_emb, audio_feat), dim=-1)
        gesture, expression = torch.split(x, m.opt.split_pos, dim=-1)
        m.opt.expCondition_gesture_only = "pred"
        audio_emb = torch.cat((audio_emb, self.track), dim=-1)
        ges_noise_t = m.encoder_ges(gesture, timesteps, audio_emb, length, person_id, add_cond, pe_type, y, block="gesture")
        m.opt.expCondition_gesture_only = None
        m.opt.gesture_only = False
        return torch.cat((ges_noise_t, torch.zeros_like(expression)), dim=-1)


def gen(tr, gd, rs, ds):
    cfg = get_config(ds)
    opt = ref_opt(cfg)
    model, _ = build_ref_model(tr, cfg, opt)
    _, ddim = build_ref_samplers(gd, rs, opt)
    B, G = BATCH[ds], cfg.split_pos
    track = make_track(cfg, B)
    given = GivenTrack(tr, model, track)
    out = {}
    # two evaluations
    inp = make_inputs(cfg, B, seed=EVAL_SEED)
    for tag, k in (("k0", 0), ("k14", 14)):
        t_model = ddim.timestep_map[k]
        c1 = float(np.float32(ddim.sqrt_recip_alphas_cumprod[k]))
        c2 = float(np.float32(ddim.sqrt_recipm1_alphas_cumprod[k]))
        shape_e = (B, cfg.n_poses, cfg.expression_dim)
        with torch.no_grad():
            eps = given(inp["x_T"], torch.full((B,), t_model, dtype=torch.long), [torch.full(shape_e, c1), torch.full(shape_e, c2)],
                        inp["audio_emb"], torch.full((B,), cfg.n_poses, dtype=torch.long), inp["person_id"],
                        {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "pe_sinu", {})
        out[f"{tag}_t"], out[f"{tag}_c1"], out[f"{tag}_c2"], out[f"{tag}_eps_ges"] = t_model, c1, c2, eps[..., :G]
    # plain ddim25 loop on the same inputs
    kw = {"audio_emb": inp["audio_emb"], "length": torch.full((B,), cfg.n_poses), "person_id": inp["person_id"],
          "add_cond": {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "y": {}, "pe_type": "pe_sinu"}
    src = SeededNoise(LOOP_NOISE)
    final, _, _ = _record_loop(ddim.ddim_sample_loop_progressive(given, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False,
                                                                 model_kwargs=kw, device=torch.device("cpu")), src, f"gesture ddim25 {ds}")
    out["ddim_draws"], out["ddim_final_ges"] = src.count, final[..., :G]
    # one out-painting window (a chain's second window): make_golden's masked inputs, default jump schedule
    kwm = _masked_kwargs(cfg, B)
    src = SeededNoise(MASKED_NOISE)
    final, _, _ = _record_loop(ddim.ddim_sample_loop_progressive_harmonize(given, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False,
                                                                           model_kwargs=kwm, device=torch.device("cpu")), src,
                               f"gesture out-painting {ds}")
    out["masked_draws"], out["masked_final_ges"] = src.count, final[..., :G]
    save(f"modality_{ds}.npz", batch=B, weight_seed=mg.WEIGHT_SEED, track_seed=TRACK_SEED, input_seed=EVAL_SEED, noise_seed=LOOP_NOISE,
         masked_input_seed=5, masked_gt_seed=17, masked_noise_seed=MASKED_NOISE, **out)


def main():
    torch.set_num_threads(8)
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="show,beat")
    only = set(ap.parse_args().only.split(","))
    tr, gd, rs, _ = mg.import_reference(with_trainer=False)
    for ds in ("show", "beat"):
        if ds in only:
            print("modality", ds); gen(tr, gd, rs, ds)


if __name__ == "__main__":
    main()
