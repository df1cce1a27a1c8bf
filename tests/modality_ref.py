"""CPU composition of the one-modality runs from the oracle's own pieces (oracle/denoiser_ref.py, oracle/sampler_ref.py): what
``UniDiffuser.set_condition(modality=...)`` computes on the device, in fp32 on the host.

  * ``gesture_eps`` / ``expression_eps``: the shared head (UniDiffuser.time_embed -> encoder_aud) and ONE motion encoder; the gesture
    encoder reads the given track where ``denoiser_ref.unidiffuser`` hands it the expression encoder's x0 estimate.  The other
    encoder's columns are 0.
  * the loops run ``sampler_ref`` at full width — full-width noise draws, so an active column receives the value it receives in the
    joint run — and the active columns are sliced out of the result: every sampler update is element-wise, so they do not depend on
    what the inactive columns hold.  The inactive columns of the returned sample are the definition's: 0, or the given track.
"""
from __future__ import annotations

from typing import Optional

import torch

from oracle import denoiser_ref as dr
from oracle import sampler_ref as sr


def _audio256(sd, cfg, t, audio_emb):
    emb_a = dr.mlp_embed(sd, "time_embed", dr.timestep_embedding(t, cfg.latent_dim))
    aud_feat = dr.decoder_layer(sd, "encoder_aud", audio_emb, None, emb_a, cfg.num_heads, None, False)
    return torch.cat((audio_emb, aud_feat), dim=-1)


def gesture_eps(sd, cfg, x, t, audio_emb, person_id, hubert, track) -> torch.Tensor:
    """eps [B, T, C] of a gesture-only evaluation: encoder_ges conditioned on ``track`` [B, T, E]; expression columns 0."""
    eps_ges = dr.motion_transformer(sd, "encoder_ges", cfg, x[..., :cfg.split_pos], t, _audio256(sd, cfg, t, audio_emb), person_id, hubert, track)
    return torch.cat((eps_ges, torch.zeros_like(x[..., cfg.split_pos:])), dim=-1)


def expression_eps(sd, cfg, x, t, audio_emb, person_id, hubert) -> torch.Tensor:
    """eps [B, T, C] of an expression-only evaluation; gesture columns 0."""
    eps_exp = dr.motion_transformer(sd, "encoder_exp", cfg, x[..., cfg.split_pos:], t, _audio256(sd, cfg, t, audio_emb), person_id, hubert, None)
    return torch.cat((torch.zeros_like(x[..., :cfg.split_pos]), eps_exp), dim=-1)


def _eps_fn(sd, cfg, audio_emb, person_id, hubert, track):
    B = audio_emb.shape[0]

    def fn(xc, t_orig, c1, c2):
        with torch.no_grad():
            t = torch.full((B,), int(t_orig), dtype=torch.long)
            if track is None:
                return expression_eps(sd, cfg, xc, t, audio_emb, person_id, hubert)
            return gesture_eps(sd, cfg, xc, t, audio_emb, person_id, hubert, track)
    return fn


def finish(cfg, x, track: Optional[torch.Tensor]) -> torch.Tensor:
    """Inactive columns of a one-modality sample: the given track (gesture mode), or 0 in the gesture columns (expression mode)."""
    G = cfg.split_pos
    if track is None:
        return torch.cat((torch.zeros_like(x[..., :G]), x[..., G:]), dim=-1)
    return torch.cat((x[..., :G], track.to(x.dtype)), dim=-1)


def ddim_loop(sd, cfg, audio_emb, person_id, hubert, track, y, noise: sr.NoiseSource, **kw) -> torch.Tensor:
    """A one-modality ddim25 loop (``track`` None = expression mode): ``sampler_ref.ddim_sample_loop`` at full width, active columns kept."""
    B, T = audio_emb.shape[:2]
    x = sr.ddim_sample_loop(_eps_fn(sd, cfg, audio_emb, person_id, hubert, track), (B, T, cfg.net_dim_pose), y, noise,
                            overlap_len=cfg.overlap_len, add_blend=cfg.add_blend, **kw)
    return finish(cfg, x, track)


def window_chain(sd, cfg, audio, person_id, hubert, track, noise_for_window) -> torch.Tensor:
    """The gesture-only out-painting chain over a stream ``[B, N, ...]``: ``sampler_ref.window_chain`` with the track cut into windows like
    the audio.  ``noise_for_window(i)`` -> the ``sampler_ref.NoiseSource`` of window ``i``."""
    step = cfg.n_poses - cfg.overlap_len
    tw = sr.get_windows(track, cfg.n_poses, step)

    def sample_window(i, a, h, y):
        return ddim_loop(sd, cfg, a, person_id, h, tw[i], y, noise_for_window(i))
    return sr.window_chain(sample_window, audio, hubert, cfg.n_poses, cfg.overlap_len, cfg.net_dim_pose)


# ---- the reference fixtures' cases (tests/golden/modality_*.npz), computed once per session and shared by the CPU and GPU tests -----------
import functools  # noqa: E402


def make_track(cfg, B, seed, frames=None) -> torch.Tensor:
    """The fixtures' given track: ~ N(0, 1) from a seeded CPU generator, [B, frames or n_poses, E]."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randn(B, cfg.n_poses if frames is None else frames, cfg.expression_dim, generator=g)


def masked_y(cfg, B, gt_seed):
    """make_golden.py's out-painting window: the first overlap_len frames pinned to seeded motion."""
    L = cfg.overlap_len
    g = torch.Generator().manual_seed(int(gt_seed))
    gt = torch.zeros(B, cfg.n_poses, cfg.net_dim_pose)
    gt[:, :L] = torch.randn(B, L, cfg.net_dim_pose, generator=g)
    mask = torch.zeros_like(gt, dtype=torch.bool)
    mask[:, :L] = True
    return {"gt": gt, "outpainting_mask": mask}


@functools.lru_cache(maxsize=2)
def fixture_case(ds: str) -> dict:
    """Inputs of tests/golden/modality_<ds>.npz regenerated from its seeds, the fixture itself, and the composition's results on them:
    ``comp_ddim`` / ``comp_masked`` [B, T, C] (expression columns = the track)."""
    from diffsheg_amd.config import get_config
    from diffsheg_amd.synthetic import make_inputs
    from util import golden, synthetic_sd
    cfg, sd, f = get_config(ds), synthetic_sd(ds), golden(f"modality_{ds}.npz")
    B = int(f["batch"])
    track = make_track(cfg, B, int(f["track_seed"]))
    inp = make_inputs(cfg, B, seed=int(f["input_seed"]))
    inp_m = make_inputs(cfg, B, seed=int(f["masked_input_seed"]))
    y = masked_y(cfg, B, int(f["masked_gt_seed"]))
    with torch.no_grad():
        src = sr.NoiseSource(seed=int(f["noise_seed"]))
        comp_ddim = ddim_loop(sd, cfg, inp["audio_emb"], inp["person_id"], inp["pretrain_aud_feat"], track, {}, src)
        src_m = sr.NoiseSource(seed=int(f["masked_noise_seed"]))
        comp_masked = ddim_loop(sd, cfg, inp_m["audio_emb"], inp_m["person_id"], inp_m["pretrain_aud_feat"], track, y, src_m,
                                jump_length=cfg.jump_length, jump_n_sample=cfg.jump_n_sample)
    return {"cfg": cfg, "sd": sd, "f": f, "B": B, "track": track, "inp": inp, "inp_m": inp_m, "y": y, "comp_ddim": comp_ddim,
            "comp_masked": comp_masked, "draws": src.i, "masked_draws": src_m.i}
