"""Boundary-2/3 parity on a real MI355X: the native sampling loops vs fixtures produced by the
imported reference with identical weights / conditioning / injected noise.

Random-weight models blow |x| up to ~1e3 over ddim25 (SURVEY §7 "numerical parity budget"), so the
end-to-end gate is relative to the output range: max|x - ref| / max|ref| <= 1e-3; per-step corner
slices are checked the same way."""
import argparse

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.synthetic import SeededNoise, make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from util import golden, gpu_model, gpu_single_model, rel_err  # noqa: E402

REL_TOL = 1e-3
# bf16 path over 25 compounding steps (random-weight model, |x| grows to ~1e3): gates at ~3x the values measured on MI355X in
# round 2 (printed by the test)
BF16_E2E_REL = 1.2e-2      # measured 3.9e-3
BF16_E2E_RMS = 1.1e-2      # measured 3.5e-3


def _kwargs(cfg, inp, y):
    B, T = inp["audio_emb"].shape[:2]
    return {"audio_emb": inp["audio_emb"], "length": torch.full((B,), T), "person_id": inp["person_id"],
            "add_cond": {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "y": y, "pe_type": "pe_sinu"}


def _check_trace(trace, f, key="step_corner"):
    corners = torch.from_numpy(f[key])
    got = trace[:, :, :3, :6].cpu()
    assert got.shape == corners.shape, (got.shape, corners.shape)
    for i in range(corners.shape[0]):
        scale = float(f["step_stats"][i][2])            # max|x| of the reference at this step
        assert float((got[i] - corners[i]).abs().max()) <= REL_TOL * max(scale, 1.0), f"step {i}"
        # whole-tensor signature (covers the un-masked frames too): mean|x| and max|x|
        assert abs(float(trace[i].abs().mean()) - float(f["step_stats"][i][1])) <= 1e-4 * float(f["step_stats"][i][1]) + 1e-6
        assert abs(float(trace[i].abs().max()) - scale) <= REL_TOL * max(scale, 1.0)


@pytest.mark.parametrize("ds", ["beat", "show"])
def test_ddim25_plain_matches_reference(ds):
    cfg = get_config(ds)
    f = golden(f"ddim25_plain_{ds}.npz")
    model = gpu_model(ds, "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B = int(f["batch"])
    inp = make_inputs(cfg, B, seed=int(f["input_seed"]))
    src = SeededNoise(int(f["noise_seed"]))
    x, trace = tr.diffusion_ddim_val.ddim_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False,
                                                      model_kwargs=_kwargs(cfg, inp, {}), noise_source=src,
                                                      return_trace=True)
    assert src.count == int(f["draws"]) == 26
    _check_trace(trace, f)
    e = rel_err(x, torch.from_numpy(f["final"]))
    print(f"[ddim25 {ds}] rel err {e:.3e}")
    assert e < REL_TOL


def _masked(cfg, f):
    B, L = int(f["batch"]), cfg.overlap_len
    inp = make_inputs(cfg, B, seed=int(f["input_seed"]))
    g = torch.Generator().manual_seed(int(f["gt_seed"]))
    gt = torch.zeros(B, cfg.n_poses, cfg.net_dim_pose)
    gt[:, :L] = torch.randn(B, L, cfg.net_dim_pose, generator=g)
    mask = torch.zeros_like(gt, dtype=torch.bool)
    mask[:, :L] = True
    return B, inp, gt, mask


@pytest.mark.parametrize("ds,jl,jn", [("show", 3, 5), ("show", 3, 2), ("beat", 3, 5)])
def test_ddim25_harmonize_matches_reference(ds, jl, jn):
    """Masked (out-painting) window: 63 denoise + 48 undo steps at (3,5).  BEAT = overlap_len 4, no CFG (has_null = 0 path
    of the denoiser), ddpm_beat_trainer.py:1006-1024."""
    cfg = get_config(ds, jump_length=jl, jump_n_sample=jn)
    f = golden(f"ddim25_harmonize_{ds}_{jl}_{jn}.npz")
    model = gpu_model(ds, "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B, inp, gt, mask = _masked(cfg, f)
    src = SeededNoise(int(f["noise_seed"]))
    x, trace = tr.diffusion_ddim_val.ddim_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False,
                                                      model_kwargs=_kwargs(cfg, inp, {"gt": gt, "outpainting_mask": mask}),
                                                      noise_source=src, return_trace=True)
    assert src.count == int(f["draws"])
    # the fixture records denoise steps only; the trace also holds the undo steps
    from diffsheg_amd.diffusion import get_schedule_jump_cjm_ddim
    times = get_schedule_jump_cjm_ddim(25, jl, jn)
    den_idx = [i for i, (a, b) in enumerate(zip(times[:-1], times[1:])) if b < a]
    _check_trace(trace[den_idx], f)
    e = rel_err(x, torch.from_numpy(f["final"]))
    print(f"[harmonize {ds} {jl},{jn}] rel err {e:.3e}")
    assert e < REL_TOL
    # out-painted frames: the masked region of the final sample is a blend that ends at gt (k=0: w_0 = 0)
    assert torch.allclose(x[:, 0].cpu(), gt[:, 0], atol=1e-5)


def test_no_resample_matches_reference():
    """--no_resample: harmonize on the 15-level list (jump_length = jump_n_sample = 1), gaussian_diffusion.py:1236-1237."""
    cfg = get_config("show", no_resample=True)
    f = golden("ddim25_noresample_show.npz")
    model = gpu_model("show", "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B, inp, gt, mask = _masked(cfg, f)
    src = SeededNoise(int(f["noise_seed"]))
    x, trace = tr.diffusion_ddim_val.ddim_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False,
                                                      model_kwargs=_kwargs(cfg, inp, {"gt": gt, "outpainting_mask": mask}),
                                                      noise_source=src, return_trace=True)
    assert src.count == int(f["draws"]) == 1 + 15 * 2
    _check_trace(trace, f)
    assert rel_err(x, torch.from_numpy(f["final"])) < REL_TOL


def test_no_repaint_matches_reference():
    """--no_repaint: a masked window goes through the PLAIN 25-step loop, but ddim_sample still blends gt in
    (gaussian_diffusion.py:1126 vs :1036): 1 + 25 * 2 draws."""
    cfg = get_config("show", no_repaint=True)
    f = golden("ddim25_norepaint_show.npz")
    model = gpu_model("show", "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B, inp, gt, mask = _masked(cfg, f)
    src = SeededNoise(int(f["noise_seed"]))
    x = tr.diffusion_ddim_val.ddim_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False,
                                               model_kwargs=_kwargs(cfg, inp, {"gt": gt, "outpainting_mask": mask}),
                                               noise_source=src)
    assert src.count == int(f["draws"]) == 51
    e = rel_err(x, torch.from_numpy(f["final"]))
    print(f"[no_repaint] rel err {e:.3e}")
    assert e < REL_TOL


def test_clip_denoised_matches_reference():
    """clip_denoised=True (gaussian_diffusion.py:575-580: pred_xstart clamped to [-1, 1] before eps is re-derived)."""
    cfg = get_config("show")
    f = golden("ddim25_clip_show.npz")
    model = gpu_model("show", "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B = int(f["batch"])
    inp = make_inputs(cfg, B, seed=int(f["input_seed"]))
    src = SeededNoise(int(f["noise_seed"]))
    x, trace = tr.diffusion_ddim_val.ddim_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=True,
                                                      model_kwargs=_kwargs(cfg, inp, {}), noise_source=src, return_trace=True)
    assert src.count == int(f["draws"]) == 26
    _check_trace(trace, f)
    assert float(x.abs().max()) <= 1.0 + 1e-6
    assert rel_err(x, torch.from_numpy(f["final"])) < REL_TOL


def test_ddpm1000_matches_reference_config1():
    """BASELINE config 1: BEAT n_poses=34, 1000 ancestral steps, batch 1."""
    cfg = get_config("beat")
    f = golden("ddpm1000_beat.npz")
    model = gpu_model("beat", "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg, ddim=False), model)
    inp = make_inputs(cfg, 1, seed=int(f["input_seed"]))
    src = SeededNoise(int(f["noise_seed"]))
    x, trace = tr.diffusion.p_sample_loop(model, (1, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False,
                                          model_kwargs=_kwargs(cfg, inp, {}), noise_source=src, return_trace=True)
    assert src.count == int(f["draws"]) == 1001
    _check_trace(trace, f)
    e = rel_err(x, torch.from_numpy(f["final"]))
    print(f"[ddpm1000 beat] rel err {e:.3e}")
    assert e < REL_TOL


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ddpm1000_show_cfg_matches_reference_config5_workload(precision):
    """Workload of BASELINE config 5: SHOW n_poses=88, CFG 1.25, all 1000 ancestral steps (p_sample_loop,
    gaussian_diffusion.py:776-841,923-974 through UniDiffuser's CFG mix, transformer.py:537-544,583-586), B = 2.
    fp32: <= 1e-3 of the output range at every recorded step and at the end.  bf16 (the precision config 5 names):
    reported, and gated on the statistics of the final sample (1000 stochastic steps decorrelate individual values)."""
    cfg = get_config("show")
    f = golden("ddpm1000_show.npz")
    model = gpu_model("show", precision)
    tr = DDPMTrainer(sampler_namespace(cfg, ddim=False), model)
    B = int(f["batch"])
    inp = make_inputs(cfg, B, seed=int(f["input_seed"]))
    src = SeededNoise(int(f["noise_seed"]))
    x, trace = tr.diffusion.p_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False,
                                          model_kwargs=_kwargs(cfg, inp, {}), noise_source=src, return_trace=True)
    assert src.count == int(f["draws"]) == 1001
    ref = torch.from_numpy(f["final"])
    e = rel_err(x, ref)
    print(f"[ddpm1000 show cfg {precision}] rel err {e:.3e}  (|x|max {float(ref.abs().max()):.3g})")
    if precision == "fp32":
        _check_trace(trace, f)
        assert e < REL_TOL
    else:
        assert torch.isfinite(x).all()
        st = f["step_stats"]
        # first 5 steps track the reference closely (errors have not compounded yet): corner values within 2 % of range
        for i in range(5):
            scale = float(st[i][2])
            assert float((trace[i][:, :3, :6].cpu() - torch.from_numpy(f["step_corner"][i])).abs().max()) <= 2e-2 * scale, i
        # end of the loop: same magnitude statistics as the reference
        assert abs(float(x.abs().mean()) - float(st[-1][1])) <= 0.05 * float(st[-1][1])
        assert e < 1.5e-2                     # measured 5.0e-3 of the output range after 1000 steps


@pytest.mark.parametrize("name", ["ddim25_eta05_show", "ddim25_eta10_show", "ddim25_eta05_masked_show"])
def test_ddim25_eta_matches_reference(name):
    """ddim_sample_loop(..., eta != 0) (gaussian_diffusion.py:1011-1032) against goldens from the imported reference: plain loop at
    eta 0.5 / 1.0 and the masked out-painting schedule at 0.5 (round 3 raised NotImplementedError here)."""
    cfg = get_config("show")
    f = golden(f"{name}.npz")
    model = gpu_model("show", "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    y = {}
    if "masked" in name:
        B, inp, gt, mask = _masked(cfg, f)
        y = {"gt": gt, "outpainting_mask": mask}
    else:
        B = int(f["batch"])
        inp = make_inputs(cfg, B, seed=int(f["input_seed"]))
    src = SeededNoise(int(f["noise_seed"]))
    x = tr.diffusion_ddim_val.ddim_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False,
                                               model_kwargs=_kwargs(cfg, inp, y), noise_source=src, eta=float(f["eta"]))
    assert src.count == int(f["draws"])
    e = rel_err(x, torch.from_numpy(f["final"]))
    print(f"[{name}] rel err {e:.3e}")
    assert e < REL_TOL
    # Philox noise: eta != 0 draws the step noise on the device (its own scratch buffer); deterministic, and not the eta = 0 result
    a = tr.diffusion_ddim_val.ddim_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False, model_kwargs=_kwargs(cfg, inp, y), seed=5, eta=0.5)
    b = tr.diffusion_ddim_val.ddim_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False, model_kwargs=_kwargs(cfg, inp, y), seed=5, eta=0.5)
    c = tr.diffusion_ddim_val.ddim_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False, model_kwargs=_kwargs(cfg, inp, y), seed=5)
    assert torch.equal(a, b) and not torch.equal(a, c) and torch.isfinite(a).all()


def test_fix_head_var_is_accepted_and_changes_nothing():
    """opt.fix_head_var = True (gaussian_diffusion.py:444,759): no effect on sampling in the reference (p_sample edits an empty slice
    of a [B, 1, 1] mask; ddim_sample never reads it) — the 50-step ancestral loop with the switch on against the reference golden
    generated WITH it on, and the refusal of unknown dataset names the reference has."""
    cfg = get_config("show")
    f = golden("ddpm50_fhv_show.npz")
    model = gpu_model("show", "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg, ddim=False, diffusion_steps=int(f["diffusion_steps"]), fix_head_var=True), model)
    B = int(f["batch"])
    inp = make_inputs(cfg, B, seed=int(f["input_seed"]))
    src = SeededNoise(int(f["noise_seed"]))
    x = tr.diffusion.p_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False, model_kwargs=_kwargs(cfg, inp, {}), noise_source=src)
    assert src.count == int(f["draws"])
    e = rel_err(x, torch.from_numpy(f["final"]))
    print(f"[ddpm50 fix_head_var] rel err {e:.3e}")
    assert e < REL_TOL
    tr2 = DDPMTrainer(sampler_namespace(cfg, ddim=False, diffusion_steps=50, fix_head_var=True, dataset_name="beat"), model)
    with pytest.raises(NotImplementedError):
        tr2.diffusion.p_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False, model_kwargs=_kwargs(cfg, inp, {}), noise_source=SeededNoise(1))


def test_bf16_ddim25_end_to_end_error_vs_reference():
    """bf16 hot path over the whole ddim25 loop against the reference golden (same noise): error relative to the output
    range, reported and gated (the fp32 path sits at ~1e-6 on the same fixture)."""
    cfg = get_config("show")
    f = golden("ddim25_plain_show.npz")
    model = gpu_model("show", "bf16")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B = int(f["batch"])
    inp = make_inputs(cfg, B, seed=int(f["input_seed"]))
    src = SeededNoise(int(f["noise_seed"]))
    x, trace = tr.diffusion_ddim_val.ddim_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False,
                                                      model_kwargs=_kwargs(cfg, inp, {}), noise_source=src, return_trace=True)
    ref = torch.from_numpy(f["final"])
    e = rel_err(x, ref)
    rms = float((x.cpu() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    worst_step = max(float((trace[i][:, :3, :6].cpu() - torch.from_numpy(f["step_corner"][i])).abs().max()) / max(float(f["step_stats"][i][2]), 1.0)
                     for i in range(trace.shape[0]))
    print(f"[ddim25 show bf16 end-to-end] max err / range = {e:.3e}, rms err / rms = {rms:.3e}, worst per-step corner / range = {worst_step:.3e}")
    assert e < BF16_E2E_REL and rms < BF16_E2E_RMS


@pytest.mark.parametrize("name", ["chain3_show", "chain_tail_show", "chain3_beat", "chain_tail_beat"])
def test_window_chain_matches_reference(name):
    ds = name.rsplit("_", 1)[1]
    cfg = get_config(ds)
    f = golden(f"{name}.npz")
    model = gpu_model(ds, "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    N = int(f["frames"])
    inp = make_inputs(cfg, 1, frames=N, seed=int(f["input_seed"]))
    srcs = []

    def src_for(i):
        srcs.append(SeededNoise(int(f["noise_seed_base"]) + i))
        return srcs[-1]
    out = tr.sample_arbitrary_len(inp["audio_emb"], inp["person_id"], {"pretrain_aud_feat": inp["pretrain_aud_feat"]},
                                  noise_source_for_window=src_for)
    assert out.shape == (1, N, cfg.net_dim_pose)
    assert [s.count for s in srcs] == list(f["draws"])
    e = rel_err(out, torch.from_numpy(f["out"]))
    print(f"[{name}] rel err {e:.3e}")
    assert e < REL_TOL


def test_fix_very_first_chain_matches_reference():
    """--fix_very_first (ddpm_show_trainer.py:885-888) through the real harness on the GPU: window 0 is out-painted from
    motions[:, n_poses - L : n_poses] (the reference's indexing), window 1 from window 0; both draw 175 tensors."""
    cfg = get_config("show")
    f = golden("chain_fvf_show.npz")
    model = gpu_model("show", "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg, fix_very_first=True), model)
    N, L = int(f["frames"]), cfg.overlap_len
    inp = make_inputs(cfg, 1, frames=N, seed=int(f["input_seed"]))
    motions = torch.randn(1, N, cfg.net_dim_pose, generator=torch.Generator().manual_seed(int(f["motions_seed"])))
    srcs = []

    def src_for(i):
        srcs.append(SeededNoise(int(f["noise_seed_base"]) + i))
        return srcs[-1]
    out = tr.sample_arbitrary_len(inp["audio_emb"], inp["person_id"], {"pretrain_aud_feat": inp["pretrain_aud_feat"]},
                                  noise_source_for_window=src_for, motions=motions)
    assert out.shape == (1, N, cfg.net_dim_pose)
    assert [s.count for s in srcs] == list(f["draws"]) == [175, 175]
    assert torch.equal(out[:, 0].cpu(), motions[:, cfg.n_poses - L])       # frame 0 of the cross-fade (addBlend) is the pinned frame itself
    e = rel_err(out, torch.from_numpy(f["out"]))
    print(f"[fix_very_first show chain] rel err {e:.3e}")
    assert e < REL_TOL


def test_same_overlap_noisy_chain_matches_reference():
    """--same_overlap_noisy (gaussian_diffusion.py:1040-1060, BEAT harness ddpm_beat_trainer.py:1006-1028): the noisy tails
    saved per level live in the native context; windows k > 0 draw no gt noise (112 draws instead of 175)."""
    cfg = get_config("beat")
    f = golden("chain_tail_beat_son.npz")
    model = gpu_model("beat", "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg, same_overlap_noisy=True), model)
    N = int(f["frames"])
    inp = make_inputs(cfg, 1, frames=N, seed=int(f["input_seed"]))
    srcs = []

    def src_for(i):
        srcs.append(SeededNoise(int(f["noise_seed_base"]) + i))
        return srcs[-1]
    out = tr.sample_arbitrary_len(inp["audio_emb"], inp["person_id"], {"pretrain_aud_feat": inp["pretrain_aud_feat"]},
                                  noise_source_for_window=src_for)
    assert out.shape == (1, N, cfg.net_dim_pose)
    assert [s.count for s in srcs] == list(f["draws"]) == [26, 112, 112]
    e = rel_err(out, torch.from_numpy(f["out"]))
    print(f"[same_overlap_noisy beat chain] rel err {e:.3e}")
    assert e < REL_TOL


def test_bf16_window_chain_with_short_tail_runs_and_is_deterministic():
    """bf16 hot path through the whole harness: three windows (88, 88, 21-frame tail), on-device Philox noise."""
    cfg = get_config("show")
    model = gpu_model("show", "bf16")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    N = 2 * 78 + 21
    inp = make_inputs(cfg, 1, frames=N, seed=12)
    args = (inp["audio_emb"], inp["person_id"], {"pretrain_aud_feat": inp["pretrain_aud_feat"]})
    a = tr.sample_arbitrary_len(*args, seed=9)
    b = tr.sample_arbitrary_len(*args, seed=9)
    assert a.shape == (1, N, cfg.net_dim_pose) and torch.isfinite(a).all()
    assert torch.equal(a, b)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_timestep_cache_is_bit_identical(precision, monkeypatch):
    """The out-painting schedule revisits levels (63 evaluations over 16 levels): the x-independent part of an evaluation
    (time / speaker / FiLM embeddings, encoder_aud, audio_proj) is restored from the per-level cache instead of being
    recomputed.  Same kernels, same inputs -> the sample must not change by a bit (DSH_LEVEL_CACHE=0 recomputes)."""
    cfg = get_config("show")
    model = gpu_model("show", precision)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B, L = 2, cfg.overlap_len
    inp = make_inputs(cfg, B, seed=21)
    gt = torch.zeros(B, cfg.n_poses, cfg.net_dim_pose)
    gt[:, :L] = torch.randn(B, L, cfg.net_dim_pose, generator=torch.Generator().manual_seed(4))
    mask = torch.zeros_like(gt, dtype=torch.bool)
    mask[:, :L] = True
    kw = _kwargs(cfg, inp, {"gt": gt, "outpainting_mask": mask})
    shape = (B, cfg.n_poses, cfg.net_dim_pose)
    a = tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, seed=11)
    monkeypatch.setenv("DSH_LEVEL_CACHE", "0")
    b = tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, seed=11)
    monkeypatch.delenv("DSH_LEVEL_CACHE")
    c = tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, seed=11)
    # default = every scheduled level computed ahead of the loop by a second instance on a side stream (level_prefetch);
    # DSH_LEVEL_PREFETCH=0 = the inline cache (compute at first use, restore afterwards)
    monkeypatch.setenv("DSH_LEVEL_PREFETCH", "0")
    d = tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, seed=11)
    monkeypatch.delenv("DSH_LEVEL_PREFETCH")
    # an un-masked window visits every level once: only the prefetch changes its launch sequence
    kw0 = _kwargs(cfg, inp, {})
    e0 = tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw0, seed=12)
    monkeypatch.setenv("DSH_LEVEL_PREFETCH", "0")
    e1 = tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw0, seed=12)
    assert torch.isfinite(a).all() and torch.isfinite(e0).all()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d) and torch.equal(e0, e1)


@pytest.mark.parametrize("ds,precision,B", [("show", "bf16", 1), ("show", "fp32", 3), ("beat", "bf16", 5), ("beat", "fp32", 1)])
def test_pipelined_encoder_chains_are_bit_identical(ds, precision, B, monkeypatch):
    """Round 6: in the launch-bound regime the expression encoder's chain E_0 -> E_1 -> ... runs on the context stream and the gesture encoder's one
    step behind on a second stream (the expression encoder never sees the gesture channels, every sampler update is element-wise:
    transformer.py:741-768, gaussian_diffusion.py:993-1063).  Same kernels on the same values: the sample must not change by a bit against the
    sequential loop (DSH_PIPE=0) — plain windows, out-painting windows (jump schedule with undo steps, RePaint noise), eta != 0, repeated runs
    (a race between the two streams would show as a mismatch)."""
    cfg = get_config(ds)
    model = gpu_model(ds, precision)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    T, Cc, L = cfg.n_poses, cfg.net_dim_pose, cfg.overlap_len
    inp = make_inputs(cfg, B, seed=31 + B)
    gt = torch.zeros(B, T, Cc)
    gt[:, :L] = torch.randn(B, L, Cc, generator=torch.Generator().manual_seed(5))
    mask = torch.zeros_like(gt, dtype=torch.bool)
    mask[:, :L] = True
    runs = {"plain": (_kwargs(cfg, inp, {}), 0.0), "outpaint": (_kwargs(cfg, inp, {"gt": gt, "outpainting_mask": mask}), 0.0),
            "eta": (_kwargs(cfg, inp, {}), 0.5)}
    for name, (kw, eta) in runs.items():
        outs = []
        for pipe in ("1", "0", "1", "1"):
            monkeypatch.setenv("DSH_PIPE", pipe)
            outs.append(tr.diffusion_ddim_val.ddim_sample_loop(model, (B, T, Cc), clip_denoised=False, model_kwargs=kw, seed=17, eta=eta))
        assert torch.isfinite(outs[0]).all(), name
        for o2 in outs[1:]:
            assert torch.equal(outs[0], o2), (name, float((outs[0] - o2).abs().max()))
    # the ancestral DDPM loop (no timestep cache: each chain computes its own head), 50 steps
    trp = DDPMTrainer(sampler_namespace(cfg, ddim=False, diffusion_steps=50), model)
    outs = []
    for pipe in ("1", "0", "1"):
        monkeypatch.setenv("DSH_PIPE", pipe)
        outs.append(trp.diffusion.p_sample_loop(model, (B, T, Cc), clip_denoised=False, model_kwargs=runs["plain"][0], seed=23))
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    monkeypatch.delenv("DSH_PIPE")


def _outpaint(cfg, B, gt_seed=5):
    T, Cc, L = cfg.n_poses, cfg.net_dim_pose, cfg.overlap_len
    gt = torch.zeros(B, T, Cc)
    gt[:, :L] = torch.randn(B, L, Cc, generator=torch.Generator().manual_seed(gt_seed))
    mask = torch.zeros_like(gt, dtype=torch.bool)
    mask[:, :L] = True
    return gt, mask


def _sample_flags():
    from diffsheg_amd import _lib
    torch.cuda.synchronize()
    got = _lib.launch_counts()
    return got["sample_graph"], got["sample_pipe"], got["sample_streams"]


@pytest.mark.parametrize("ds,precision,B", [("show", "bf16", 2), ("beat", "fp32", 3)])
def test_pipelined_outpainting_with_eta_is_bit_identical(ds, precision, B, monkeypatch):
    """An out-painting window (jump schedule with undo steps, RePaint gt noise) at eta = 0.5: every DDIM step of either encoder chain draws
    both the step's own noise and the gt noise, so both noise scratch buffers of both chains are live in one step.  Pipelined and
    sequential loops give the same bits."""
    cfg = get_config(ds)
    model = gpu_model(ds, precision)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    gt, mask = _outpaint(cfg, B)
    kw = _kwargs(cfg, make_inputs(cfg, B, seed=43 + B), {"gt": gt, "outpainting_mask": mask})
    outs = []
    for pipe in ("1", "0", "1"):
        monkeypatch.setenv("DSH_PIPE", pipe)
        outs.append(tr.diffusion_ddim_val.ddim_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False, model_kwargs=kw,
                                                           seed=19, eta=0.5).clone())
        assert _sample_flags()[1] == int(pipe), pipe
    monkeypatch.delenv("DSH_PIPE")
    assert torch.isfinite(outs[0]).all()
    for o2 in outs[1:]:
        assert torch.equal(outs[0], o2), float((outs[0] - o2).abs().max())


def test_pipelined_ddpm_above_the_graph_range_is_bit_identical(monkeypatch):
    """SHOW bf16, B = 47 (4 136 token rows: one batch above DSH_GRAPH_ROWS = 4 096), the 50-step ancestral loop with row keys: the two encoder
    chains evaluate eagerly, each computing its own head.  Both runs are one unsplit batch of the same shape, so every launch runs the same
    kernel on the same values."""
    cfg = get_config("show")
    model = gpu_model("show", "bf16")
    tr = DDPMTrainer(sampler_namespace(cfg, ddim=False, diffusion_steps=50), model)
    B = 47
    kw = _kwargs(cfg, make_inputs(cfg, B, seed=47), {})
    outs = {}
    for pipe in ("1", "0"):
        monkeypatch.setenv("DSH_PIPE", pipe)
        outs[pipe] = tr.diffusion.p_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False, model_kwargs=kw, seed=29,
                                                row_keys=list(range(B))).clone()
        assert _sample_flags() == (0, int(pipe), 1), pipe
    monkeypatch.delenv("DSH_PIPE")
    assert torch.isfinite(outs["1"]).all()
    assert torch.equal(outs["1"], outs["0"]), float((outs["1"] - outs["0"]).abs().max())


def test_sub_batch_streams_share_the_noise_scratch_by_offset(monkeypatch):
    """SHOW fp32, B = 50 (4 400 token rows: two sub-batch streams), an out-painting window at eta = 0.5 with one Philox stream per row: both
    sub-batches draw both noises of a step into their own slices of the shared scratch buffers.  Rows at the batch ends and on either side of
    the split equal the row sampled alone (the gate of test_gpu_dispatch_sweep.py's loops: LOOP_TOL["fp32"])."""
    monkeypatch.setenv("DSH_PIPE", "0")
    cfg = get_config("show")
    model = gpu_model("show", "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B, shape1 = 50, (1, cfg.n_poses, cfg.net_dim_pose)
    inp = make_inputs(cfg, B, seed=53)
    gt, mask = _outpaint(cfg, B)
    full = tr.diffusion_ddim_val.ddim_sample_loop(model, (B,) + shape1[1:], clip_denoised=False, seed=31, eta=0.5, row_keys=list(range(B)),
                                                  model_kwargs=_kwargs(cfg, inp, {"gt": gt, "outpainting_mask": mask})).clone()
    assert _sample_flags()[2] == 2
    assert torch.isfinite(full).all()
    for b in (0, 24, 25, 49):
        kw = _kwargs(cfg, {k: v[b:b + 1] for k, v in inp.items()}, {"gt": gt[b:b + 1], "outpainting_mask": mask[b:b + 1]})
        solo = tr.diffusion_ddim_val.ddim_sample_loop(model, shape1, clip_denoised=False, seed=31, eta=0.5, row_keys=[b], model_kwargs=kw)
        e = rel_err(solo[0], full[b])
        print(f"[two sub-batch streams, out-painting, eta 0.5] row {b} vs the row sampled alone: rel err {e:.3e}")
        assert e < 1e-5, b
    monkeypatch.delenv("DSH_PIPE")


def test_philox_mode_runs_and_is_seed_deterministic():
    cfg = get_config("show")
    model = gpu_model("show", "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    inp = make_inputs(cfg, 2, frames=40, seed=8)
    kw = _kwargs(cfg, inp, {})
    a = tr.diffusion_ddim_val.ddim_sample_loop(model, (2, 40, cfg.net_dim_pose), clip_denoised=False, model_kwargs=kw, seed=5)
    b = tr.diffusion_ddim_val.ddim_sample_loop(model, (2, 40, cfg.net_dim_pose), clip_denoised=False, model_kwargs=kw, seed=5)
    c = tr.diffusion_ddim_val.ddim_sample_loop(model, (2, 40, cfg.net_dim_pose), clip_denoised=False, model_kwargs=kw, seed=6)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_batch_rows_are_independent():
    """Size-independent property behind the multi-GPU sharding: sampling a batch equals
    sampling its rows separately (same per-row conditioning and noise)."""
    cfg = get_config("show")
    model = gpu_model("show", "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B, T = 4, 32
    inp = make_inputs(cfg, B, frames=T, seed=12)
    xT = inp["x_T"]

    class Rows:
        def __init__(self, rows): self.g = torch.Generator().manual_seed(77); self.rows = rows
        def randn(self, shape): return torch.randn(B, *shape[1:], generator=self.g)[self.rows]
    full = tr.diffusion_ddim_val.ddim_sample_loop(model, (B, T, cfg.net_dim_pose), noise=xT, clip_denoised=False,
                                                  model_kwargs=_kwargs(cfg, inp, {}), noise_source=Rows(slice(None)))
    sub_inp = {k: v[1:3] for k, v in inp.items()}
    part = tr.diffusion_ddim_val.ddim_sample_loop(model, (2, T, cfg.net_dim_pose), noise=xT[1:3], clip_denoised=False,
                                                  model_kwargs=_kwargs(cfg, sub_inp, {}), noise_source=Rows(slice(1, 3)))
    assert rel_err(part, full[1:3]) < 1e-5


# ---- (f)-4: single MotionTransformer (opt.unidiffuser = False, runner.py:46-57) -------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_single_motion_transformer_matches_reference(precision):
    """One MotionTransformer over all 232 channels: evaluations through the reference call signature
    model(x, t, audio_emb, length, person_id, add_cond, pe_type, y), the plain ddim25 loop and one out-painting window, vs the
    fixture generated from the reference's own MotionTransformer / SpacedDiffusion (gaussian_diffusion.py:527-536: no
    sqrt_alphas for this model)."""
    f = golden("single_transformer_show.npz")
    model = gpu_single_model(precision)
    cfg = model.cfg
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B = int(f["batch"])
    inp = make_inputs(cfg, B, seed=int(f["input_seed"]))
    tol_eval, tol_loop = (1e-3, REL_TOL) if precision == "fp32" else (6e-2, BF16_E2E_REL)
    for tag in ("k3", "k20"):
        eps = model(inp["x_T"].cuda(), torch.full((B,), int(f[f"{tag}_t"]), dtype=torch.long), inp["audio_emb"],
                    torch.full((B,), cfg.n_poses), inp["person_id"], {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "pe_sinu", {})
        e = float((eps.cpu() - torch.from_numpy(f[f"{tag}_eps"])).abs().max())
        print(f"[single {precision} eval {tag}] max abs err {e:.3e}")
        assert e < tol_eval
    shape = (B, cfg.n_poses, cfg.net_dim_pose)
    src = SeededNoise(int(f["noise_seed"]))
    x, trace = tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=_kwargs(cfg, inp, {}),
                                                      noise_source=src, return_trace=True)
    assert src.count == int(f["draws"]) == 26
    if precision == "fp32":
        _check_trace(trace, f)
    e = rel_err(x, torch.from_numpy(f["final"]))
    print(f"[single {precision} ddim25] rel err {e:.3e}")
    assert e < tol_loop
    # out-painting window (63 evaluations + 48 undo steps; timestep cache + graph replay on this model too)
    inp2 = make_inputs(cfg, B, seed=int(f["masked_input_seed"]))
    L = cfg.overlap_len
    gt = torch.zeros(shape)
    gt[:, :L] = torch.randn(B, L, cfg.net_dim_pose, generator=torch.Generator().manual_seed(int(f["masked_gt_seed"])))
    mask = torch.zeros_like(gt, dtype=torch.bool)
    mask[:, :L] = True
    src2 = SeededNoise(int(f["masked_noise_seed"]))
    xm = tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False,
                                                model_kwargs=_kwargs(cfg, inp2, {"gt": gt, "outpainting_mask": mask}), noise_source=src2)
    assert src2.count == int(f["masked_draws"])
    e = rel_err(xm, torch.from_numpy(f["masked_final"]))
    print(f"[single {precision} out-painting window] rel err {e:.3e}")
    assert e < tol_loop
