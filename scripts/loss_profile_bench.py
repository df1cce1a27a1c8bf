#!/usr/bin/env python3
"""What the denoising losses cost around the evaluations they score, SHOW bf16 at B = 1, 100 and 950:

  denoising_losses          noise, q_sample, one evaluation, the loss kernel; one timestep per clip drawn by the uniform sampler
  loss_profile(levels=25)   the same per level of the ddim25 spacing, one timestep for the whole batch per level, condition set once
each against
  (a) the evaluations alone: the same model calls on ready-made x_t / t / coefficients, nothing around them;
  (b) what a user would write today: torch.randn on the device, the existing q_sample, the evaluation, then the same terms as plain torch
      ops on the device with .item() per term.

Wall time of the host around work that ends in a device synchronise, median of --steps repetitions after a warm-up of every shape.  Prints
one JSON line per batch size with both ratios (ours / a, ours / b); --out also writes them to a file.

Usage:  python scripts/loss_profile_bench.py [--batches 1,100,950] [--steps 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.model import UniDiffuser  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from diffsheg_amd.weights import make_synthetic_state_dict  # noqa: E402

DEV = "cuda:0"
BETA = 0.1


def torch_terms(eps, noise, x_t, x0, c1, c2) -> dict:
    """(b): backward_G's lines in torch on the device, every logged number fetched with .item() as the reference's trainer does."""
    frame = ((eps - noise) ** 2).mean(dim=-1)
    lmp = 1000 * frame.mean()
    out = {"loss_model_pred": lmp.item()}
    xp = c1.view(-1, 1, 1) * x_t - c2.view(-1, 1, 1) * eps
    vel = (((xp[:, :-1] - xp[:, 1:]) - (x0[:, :-1] - x0[:, 1:])) ** 2).mean(dim=-1).mean()
    out["loss_vel_rec"] = (100 * vel).item()
    lx0 = 100 * torch.nn.functional.smooth_l1_loss(x0 / BETA, xp / BETA) * BETA
    out["loss_x0_rec"] = lx0.item()
    out["final_loss"] = (lmp + vel + lx0).item()
    out["mse"] = frame.mean(dim=-1)
    out["xstart_mse"] = ((xp - x0) ** 2).mean(dim=(1, 2))
    return out


def timed(fn, steps: int) -> float:
    fn()                                                   # warm-up of this shape
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def run(B: int, steps: int, model, cfg) -> dict:
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    small = make_inputs(cfg, min(B, 64), seed=3)
    rep = (B + 63) // 64
    audio = small["audio_emb"].repeat(rep, 1, 1)[:B].to(DEV).contiguous()
    hubert = small["pretrain_aud_feat"].repeat(rep, 1, 1)[:B].to(DEV).contiguous()
    pid = torch.zeros(B, cfg.style_dim, device=DEV)
    pid[torch.arange(B), torch.arange(B) % cfg.style_dim] = 1.0
    x0 = torch.randn(B, cfg.n_poses, cfg.net_dim_pose, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))
    add = {"pretrain_aud_feat": hubert}
    kw = {"audio_emb": audio, "length": torch.full((B,), cfg.n_poses), "person_id": pid, "add_cond": add, "y": None, "pe_type": "pe_sinu"}

    def inputs_at(diff, ts, seed):
        """x_t, the model's timesteps and the coefficients of one evaluation, ready on the device"""
        out = diff.training_losses(model, x0, ts, kw, seed=seed)
        c1 = torch.from_numpy(diff.sqrt_recip_alphas_cumprod[ts]).float().to(DEV)
        c2 = torch.from_numpy(diff.sqrt_recipm1_alphas_cumprod[ts]).float().to(DEV)
        tm = torch.tensor([diff.timestep_map[v] for v in ts]).to(DEV)
        return out["x_t"], out["target"], tm, c1, c2

    def by_hand(diff, ts, tm, c1, c2):
        noise = torch.randn_like(x0)
        x_t = diff.q_sample(x0, ts, noise=noise)
        return torch_terms(evaluate(x_t, tm, c1, c2), noise, x_t, x0, c1, c2)

    def evaluate(x_t, tm, c1, c2):
        return model(x_t, tm, sqrt_alphas=[c1, c2], audio_emb=audio, length=kw["length"], person_id=pid, add_cond=add, pe_type="pe_sinu", y=None)

    # ---- one call, one timestep per clip ----
    ts = [int(v) for v in tr.sampler.sample(B, "cpu", np.random.RandomState(5))[0]]
    one = inputs_at(tr.diffusion, ts, 21)
    t_ours = timed(lambda: tr.denoising_losses(audio, x0, pid, add, t=ts, seed=21), steps)
    t_eval = timed(lambda: evaluate(one[0], *one[2:]), steps)
    t_torch = timed(lambda: by_hand(tr.diffusion, ts, *one[2:]), steps)
    # ---- the 25-level profile ----
    ddim = tr.diffusion_ddim_val
    levels = list(range(ddim.num_timesteps))
    per = [inputs_at(ddim, [k] * B, 100 + k) for k in levels]
    p_ours = timed(lambda: tr.loss_profile(audio, x0, pid, add, seed=3), steps)
    p_eval = timed(lambda: [evaluate(v[0], *v[2:]) for v in per], steps)
    p_torch = timed(lambda: [by_hand(ddim, [k] * B, *per[k][2:]) for k in levels], steps)
    return {"batch": B, "frames": cfg.n_poses, "precision": "bf16", "steps": steps,
            "denoising_losses_s": t_ours, "evaluation_alone_s": t_eval, "torch_terms_with_item_s": t_torch,
            "denoising_losses_over_evaluation": t_ours / t_eval, "denoising_losses_over_torch_terms": t_ours / t_torch,
            "loss_profile25_s": p_ours, "evaluations25_alone_s": p_eval, "torch_terms25_with_item_s": p_torch,
            "loss_profile_over_evaluations": p_ours / p_eval, "loss_profile_over_torch_terms": p_ours / p_torch}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,100,950")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = get_config("show")
    model = UniDiffuser(cfg, make_synthetic_state_dict(cfg, 1234), device=DEV, precision="bf16")
    lines = []
    for B in (int(v) for v in args.batches.split(",")):
        lines.append(json.dumps(run(B, args.steps, model, cfg)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
