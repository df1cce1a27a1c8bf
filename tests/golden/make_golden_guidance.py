#!/usr/bin/env python3
"""Guidance-scale fixtures: the imported reference (CPU) at runtime values of ``opt.cond_scale``, which the reference
reads on every forward (models/transformer.py:537, :586).  Reuses make_golden.py's helpers; same rules (inputs are seeds,
only expected outputs are stored).

  guidance_show.npz          eval_show's inputs (B = 2, T = 88, weight seed 1234, input seed 3) at cond_scale 1.0 / 1.15 / 2.0,
                             ddim25 levels k0 and k14: eps as its two encoders' mixed outputs, eps_ges [.., :dim_pose] and
                             eps_exp [.., dim_pose:] (eps = cat(eps_ges, eps_exp), transformer.py:770; stored once, not twice,
                             to keep the file under 1 MiB)
  ddim25_guidance_show.npz   a plain ddim25 loop at cond_scale 1.15 (B = 2, noise seed 100), recorded as gen_ddim_plain does

Usage:  python tests/golden/make_golden_guidance.py
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

SCALES = {"s100": 1.0, "s115": 1.15, "s200": 2.0}


def gen_guidance_eval(tr, gd, rs):
    cfg = get_config("show")
    opt = ref_opt(cfg)
    model, _ = build_ref_model(tr, cfg, opt)
    _, ddim = build_ref_samplers(gd, rs, opt)
    B = 2
    inp = make_inputs(cfg, B, seed=3)
    out = {}
    for tag, k in (("k0", 0), ("k14", 14)):
        t_model = ddim.timestep_map[k]
        c1 = float(np.float32(ddim.sqrt_recip_alphas_cumprod[k]))
        c2 = float(np.float32(ddim.sqrt_recipm1_alphas_cumprod[k]))
        out[f"{tag}_t"], out[f"{tag}_c1"], out[f"{tag}_c2"] = t_model, c1, c2
        shape_e = (B, cfg.n_poses, cfg.expression_dim)
        sa = [torch.full(shape_e, c1), torch.full(shape_e, c2)]
        for st, s in SCALES.items():
            opt.cond_scale = s                      # read by the model on this forward (transformer.py:537)
            inter = {}
            h1 = model.encoder_exp.register_forward_hook(lambda m, i, o: inter.__setitem__("eps_exp", o.detach().clone()))
            with torch.no_grad():
                eps = model(inp["x_T"], torch.full((B,), t_model, dtype=torch.long), sa, inp["audio_emb"],
                            torch.full((B,), cfg.n_poses, dtype=torch.long), inp["person_id"],
                            {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "pe_sinu", {})
            h1.remove()
            assert torch.equal(eps[..., cfg.split_pos:], inter["eps_exp"])
            out[f"{tag}_{st}_eps_ges"] = eps[..., :cfg.split_pos]
            out[f"{tag}_{st}_eps_exp"] = inter["eps_exp"]
    opt.cond_scale = cfg.cond_scale
    save("guidance_show.npz", batch=B, input_seed=3, weight_seed=mg.WEIGHT_SEED, scales=np.array(list(SCALES.values())), **out)


def gen_guidance_ddim(tr, gd, rs, scale=1.15):
    cfg = get_config("show")
    opt = ref_opt(cfg)
    opt.cond_scale = scale
    model, _ = build_ref_model(tr, cfg, opt)
    _, ddim = build_ref_samplers(gd, rs, opt)
    B = 2
    inp = make_inputs(cfg, B, seed=3)
    src = SeededNoise(100)
    stats, corners, x0c = [], [], []
    kw = {"audio_emb": inp["audio_emb"], "length": torch.full((B,), cfg.n_poses), "person_id": inp["person_id"],
          "add_cond": {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "y": {}, "pe_type": "pe_sinu"}
    t0 = time.time()
    with patched_noise(src), torch.no_grad():
        final = None
        for o in ddim.ddim_sample_loop_progressive(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False,
                                                   model_kwargs=kw, device=torch.device("cpu")):
            s, c = step_stats(o["sample"])
            stats.append(s); corners.append(c); x0c.append(step_stats(o["pred_xstart"])[1])
            final = o["sample"]
    print(f"  ddim25 cond_scale {scale}: {time.time()-t0:.1f}s, draws={src.count}, |x|max={final.abs().max():.3g}")
    save("ddim25_guidance_show.npz", batch=B, input_seed=3, noise_seed=100, cond_scale=scale, draws=src.count, final=final,
         step_stats=np.stack(stats), step_corner=np.stack(corners), x0_corner=np.stack(x0c))


def main():
    torch.set_num_threads(8)
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="eval,ddim")
    only = set(ap.parse_args().only.split(","))
    tr, gd, rs, _ = mg.import_reference(with_trainer=False)
    if "eval" in only:
        print("guidance eval"); gen_guidance_eval(tr, gd, rs)
    if "ddim" in only:
        print("guidance ddim"); gen_guidance_ddim(tr, gd, rs)


if __name__ == "__main__":
    main()
