"""The denoising losses end to end on a real MI355X: GaussianDiffusion.training_losses / DDPMTrainer.denoising_losses / loss_profile against the
fixtures the imported reference produced (tests/golden/losses_*.npz, make_golden_losses.py), against their own building blocks bit for bit, bf16
against fp32, and ragged batches against the rows alone.

Tolerances: no number of a loss is fixed here.  Every gate is the project's existing bar on eps — fp32 |eps - reference| < FP32_ATOL, bf16
BF16_MAX / BF16_RMS (tests/test_gpu_eval.py) — carried through the formula.  With d = eps - noise and an eps that moves by at most A per element:
    (eps - noise)^2 terms      mean((d + delta)^2) - mean(d^2) <= 2 A mean|d| + A^2            (rms form: 2 rms(d) R + R^2, Cauchy-Schwarz)
    x0_pred = c1 x_t - c2 eps  moves by at most c2 A, a frame difference of it by 2 c2 A
    velocity                   mean(2 |dv| 2 c2 A + (2 c2 A)^2)
    Huber                      smooth_l1 is 1-Lipschitz: beta * mean(c2 A / beta) = A mean(c2)
d, dv and c2 come from the fixture (or the run compared against) at each row's own t; at t = 999 c2 ~ 158.  On top comes ROUND: the kernel's
float32 differences against a float64 evaluation of the same formula, a few float32 ulp of the value."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import losses_ref as LR  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.synthetic import SeededNoise, make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, level_seed, sampler_namespace  # noqa: E402
from diffsheg_amd import _lib  # noqa: E402
from util import assert_split_ran, golden, gpu_model  # noqa: E402

DEV = "cuda:0"
FP32_ATOL = 1e-3                      # tests/test_gpu_eval.py
BF16_MAX, BF16_RMS = 6e-2, 1.5e-2     # tests/test_gpu_eval.py
ROUND = 8 * 2.0 ** -23                # float32 differences against float64: relative, far below every propagated bound
CASES = {"show": ("show", {}), "show_cs1": ("show", {"cond_scale": 1.0}), "beat": ("beat", {})}


def setup(tag, precision="fp32", model_over=None):
    f = golden(f"losses_{tag}.npz")
    ds, over = CASES[tag]
    over = over if model_over is None else model_over
    cfg = get_config(ds, **over)
    model = gpu_model(ds, precision, **over)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B, T, C = int(f["batch"]), int(f["frames"]), cfg.net_dim_pose
    inp = make_inputs(cfg, B, seed=int(f["input_seed"]))
    x0 = torch.randn(B, T, C, generator=torch.Generator().manual_seed(int(f["x0_seed"])))
    noise = SeededNoise(int(f["noise_seed"])).randn((B, T, C))
    t = [int(v) for v in f["t"]]
    args = (inp["audio_emb"].to(DEV), x0.to(DEV), inp["person_id"].to(DEV), {"pretrain_aud_feat": inp["pretrain_aud_feat"].to(DEV)})
    return f, cfg, model, tr, args, x0, noise, t


def kwargs_of(args, T, length=None):
    return {"audio_emb": args[0], "length": torch.full((args[0].shape[0],), T) if length is None else length, "person_id": args[2],
            "add_cond": args[3], "y": {}, "pe_type": "pe_sinu"}


def bounds(pred, noise, x_t, x0, c1, c2, A, beta, R=None):
    """How far each reported number can move when every element of eps moves by at most A[b] (rms over the batch at most R, if given) from
    `pred` — the derivation in the module docstring; float64 numpy, rows of full length."""
    pred, noise, x_t, x0 = (np.asarray(v, dtype=np.float64) for v in (pred, noise, x_t, x0))
    B, T, C = pred.shape
    A = np.broadcast_to(np.asarray(A, dtype=np.float64), (B,)).reshape(B, 1, 1)
    c1, c2 = np.asarray(c1, dtype=np.float64).reshape(B, 1, 1), np.asarray(c2, dtype=np.float64).reshape(B, 1, 1)
    d = np.abs(pred - noise)
    xp = c1 * x_t - c2 * pred
    dv = np.abs((xp[:, :-1] - xp[:, 1:]) - (x0[:, :-1] - x0[:, 1:]))
    el = 2 * A * d + A * A                                      # per element of (eps - noise)^2
    ev = 4 * c2 * A * dv + (2 * c2 * A) ** 2                    # per element of the velocity term
    b = {"frame_mse": el.mean(-1), "mse": el.mean((1, 2)), "loss_model_pred": 1000 * el.mean(), "loss_vel_rec": 100 * ev.mean(),
         "loss_x0_rec": 100 * float((c2 * A).mean())}
    if R is not None:
        b["loss_model_pred"] = min(b["loss_model_pred"], 1000 * (2 * np.sqrt((d * d).mean()) * R + R * R))
    b["final_loss"] = b["loss_model_pred"] + b["loss_vel_rec"] / 100 + b["loss_x0_rec"]
    return b


def check(what, got, want, bound):
    got, want, bound = (np.asarray(v, dtype=np.float64) for v in (got, want, bound))
    dist = np.abs(got - want)
    gate = bound + ROUND * np.abs(want)
    k = int(np.argmax(dist / gate))
    print(f"[losses {what}] relative distance {float((dist / np.abs(want)).max()):.3e}, gate {float((gate / np.abs(want)).flat[k]):.3e} "
          f"(worst distance / gate {float((dist / gate).max()):.3f})")
    assert (dist <= gate).all(), (what, float(dist.flat[k]), float(gate.flat[k]))


def coefficients(diff, t):
    return (torch.from_numpy(diff.sqrt_recip_alphas_cumprod[t]).float(), torch.from_numpy(diff.sqrt_recipm1_alphas_cumprod[t]).float())


@pytest.mark.parametrize("tag", list(CASES))
def test_losses_fp32_match_the_reference_fixture(tag):
    f, cfg, model, tr, args, x0, noise, t = setup(tag)
    T = int(f["frames"])
    out = tr.diffusion.training_losses(model, args[1], t, kwargs_of(args, T), noise=noise.to(DEV))
    tl = tr.denoising_losses(*args, t=t, noise=noise.to(DEV))
    c1, c2 = coefficients(tr.diffusion, t)
    x_t = out["x_t"].cpu()
    eps_err = float((out["pred"].cpu() - torch.from_numpy(f["pred"])).abs().max())
    print(f"[losses {tag}] max |eps - reference| = {eps_err:.3e} (bar {FP32_ATOL:g})")
    assert eps_err < FP32_ATOL
    b = bounds(f["pred"], noise, x_t, x0, c1, c2, FP32_ATOL, float(f["huber_beta"]))
    check(f"{tag} mse", out["mse"].cpu(), f["mse"], b["mse"])
    check(f"{tag} frame_mse", out["frame_mse"].cpu(), f["frame_mse"], b["frame_mse"])
    for k in LR.SCALARS:
        check(f"{tag} {k}", tl[k].cpu(), float(f[k]), b[k])
        assert tl[k].dim() == 0 and tl[k].is_cuda and torch.equal(tl[k], out["scalars"][k])
    assert torch.equal(tl["row_terms"], out["row_terms"]) and torch.equal(tl["frame_mse"], out["frame_mse"])
    # the dict's other keys
    assert out["target_x0"] is args[1] and torch.equal(out["target"].cpu(), noise)
    assert tuple(out["row_terms"].shape) == (3, 7) and out["row_terms"].dtype == torch.float64
    # the kernel's numbers against a float64 evaluation of the formulas on the eps this run produced: round-off only
    rows = LR.row_terms_f64(out["pred"].cpu(), noise, x_t, x0, c1, c2, cfg.split_pos, float(f["huber_beta"]))
    got = out["row_terms"].cpu().numpy()
    assert np.abs(got[:, :5] - rows[:, :5]).max() <= 1e-5 * np.abs(rows[:, :5]).max() and np.array_equal(got[:, 5:], rows[:, 5:])


def setup_split(B=16, ds="beat"):
    """precision "bf16x3" above the 512-row limit of the split-bf16 loop (BEAT B = 16: 544 rows; the fixtures' batches are below it): seeded
    inputs with a timestep per clip that reaches both ends of the schedule, and the fp32 model beside it."""
    cfg = get_config(ds)
    T, C = cfg.n_poses, cfg.net_dim_pose
    inp = make_inputs(cfg, B, seed=91)
    x0 = torch.randn(B, T, C, generator=torch.Generator().manual_seed(92))
    noise = SeededNoise(93).randn((B, T, C))
    t = [0, 999] + [(61 * i + 7) % 1000 for i in range(B - 2)]
    args = (inp["audio_emb"].to(DEV), x0.to(DEV), inp["person_id"].to(DEV), {"pretrain_aud_feat": inp["pretrain_aud_feat"].to(DEV)})
    trs = {p: DDPMTrainer(sampler_namespace(cfg), gpu_model(ds, p)) for p in ("bf16x3", "fp32")}
    return cfg, trs, args, x0, noise, t


def test_losses_on_the_split_loop_against_float64_on_the_fp32_models_eps():
    """training_losses with precision "bf16x3": every reported number against losses_ref.py in float64 evaluated on the eps the FP32 model
    produced for the same x_t, under the gates of the fixture test - eps within FP32_ATOL of it, carried through the formulas (bounds())."""
    cfg, trs, args, x0, noise, t = setup_split()
    T, C = cfg.n_poses, cfg.net_dim_pose
    _lib.launch_counts(reset=True)
    out = trs["bf16x3"].diffusion.training_losses(trs["bf16x3"].encoder, args[1], t, kwargs_of(args, T), noise=noise.to(DEV))
    torch.cuda.synchronize()
    assert_split_ran(_lib.launch_counts(), "training_losses")
    out32 = trs["fp32"].diffusion.training_losses(trs["fp32"].encoder, args[1], t, kwargs_of(args, T), noise=noise.to(DEV))
    assert torch.equal(out["x_t"], out32["x_t"])                                 # (q_sample does not depend on the precision of the Linears)
    pred32, x_t = out32["pred"].cpu(), out["x_t"].cpu()
    eps_err = float((out["pred"].cpu() - pred32).abs().max())
    print(f"[measure] losses beat bf16x3 B=16: max |eps - eps(fp32)| = {eps_err:.3e} (bar {FP32_ATOL:g})")
    assert eps_err < FP32_ATOL and not torch.equal(out["pred"], out32["pred"])
    c1, c2 = coefficients(trs["bf16x3"].diffusion, t)
    b = bounds(pred32, noise, x_t, x0, c1, c2, FP32_ATOL, LR.HUBER_BETA)
    rows32 = LR.row_terms_f64(pred32, noise, x_t, x0, c1, c2, cfg.split_pos)
    want = LR.scalars_f64(rows32, C)
    fm = LR.frame_mse_f64(pred32, noise)
    check("bf16x3 mse", out["mse"].cpu(), fm.mean(-1), b["mse"])
    check("bf16x3 frame_mse", out["frame_mse"].cpu(), fm, b["frame_mse"])
    for k in LR.SCALARS:
        check(f"bf16x3 {k}", out["scalars"][k].cpu(), want[k], b[k])
    # the kernel's numbers against a float64 evaluation of the formulas on the eps THIS run produced: round-off only
    rows = LR.row_terms_f64(out["pred"].cpu(), noise, x_t, x0, c1, c2, cfg.split_pos)
    got = out["row_terms"].cpu().numpy()
    assert np.abs(got[:, :5] - rows[:, :5]).max() <= 1e-5 * np.abs(rows[:, :5]).max() and np.array_equal(got[:, 5:], rows[:, 5:])


def test_losses_are_composed_of_the_existing_calls_bit_for_bit():
    f, cfg, model, tr, args, x0, noise, t = setup("show")
    _composed_of_the_existing_calls(model, tr, args, t, int(f["frames"]))


def test_losses_on_the_split_loop_are_composed_of_the_existing_calls_bit_for_bit():
    cfg, trs, args, x0, noise, t = setup_split()
    _lib.launch_counts(reset=True)
    _composed_of_the_existing_calls(trs["bf16x3"].encoder, trs["bf16x3"], args, t, cfg.n_poses)
    assert_split_ran(_lib.launch_counts(), "composition")


def _composed_of_the_existing_calls(model, tr, args, t, T):
    diff = tr.diffusion
    kw = kwargs_of(args, T)
    out = diff.training_losses(model, args[1], t, kw, seed=77)
    # x_t: what q_sample draws itself from the same seed; and the noise handed out is the noise that made it
    assert torch.equal(out["x_t"], diff.q_sample(args[1], t, seed=77))
    assert torch.equal(out["x_t"], diff.q_sample(args[1], t, noise=out["target"]))
    assert not torch.equal(out["x_t"], diff.training_losses(model, args[1], t, kw, seed=78)["x_t"])
    # pred: the model called directly on that x_t
    c1, c2 = coefficients(diff, t)
    direct = model(out["x_t"], torch.tensor([diff.timestep_map[v] for v in t]).to(DEV), sqrt_alphas=[c1.to(DEV), c2.to(DEV)], **kw)
    assert torch.equal(out["pred"], direct)
    # a SpacedDiffusion indexes its own tables and hands the model the original timestep
    ddim = tr.diffusion_ddim_val
    lv = [(0, 12, 24)[b % 3] for b in range(len(t))]
    o2 = ddim.training_losses(model, args[1], lv, kw, noise=out["target"])
    k1, k2 = coefficients(ddim, lv)
    direct = model(o2["x_t"], torch.tensor([(0, 480, 960)[b % 3] for b in range(len(t))]).to(DEV), sqrt_alphas=[k1.to(DEV), k2.to(DEV)], **kw)
    assert torch.equal(o2["pred"], direct) and torch.equal(o2["x_t"], ddim.q_sample(args[1], lv, noise=out["target"]))


def test_cond_scale_one_on_the_call_scores_the_conditional_model():
    f, cfg, model, tr, args, x0, noise, t = setup("show_cs1", model_over={})      # the classifier-free model at its cond_scale 1.25 ...
    assert model.cfg.cond_scale == 1.25 and model.guidance_scale is None
    T = int(f["frames"])
    out = tr.diffusion.training_losses(model, args[1], t, kwargs_of(args, T), noise=noise.to(DEV), cond_scale=1.0)      # ... asked for 1
    assert model.guidance_scale is None                                            # the call's scale does not stick
    c1, c2 = coefficients(tr.diffusion, t)
    b = bounds(f["pred"], noise, out["x_t"].cpu(), x0, c1, c2, FP32_ATOL, float(f["huber_beta"]))
    check("cond_scale=1 mse", out["mse"].cpu(), f["mse"], b["mse"])
    for k in LR.SCALARS:
        check(f"cond_scale=1 {k}", out["scalars"][k].cpu(), float(f[k]), b[k])
    guided = golden("losses_show.npz")
    assert abs(float(out["scalars"]["loss_model_pred"]) - float(guided["loss_model_pred"])) > 10 * b["loss_model_pred"]


@pytest.mark.parametrize("tag", ["show", "beat"])
def test_losses_bf16_against_fp32_on_the_same_inputs(tag):
    f, cfg, model32, tr32, args, x0, noise, t = setup(tag)
    _, _, model16, tr16, _, _, _, _ = setup(tag, "bf16")
    if tag == "show":
        assert (int(f["batch"]), int(f["frames"])) == (3, 88)
    T = int(f["frames"])
    nz = noise.to(DEV)
    o32 = tr32.diffusion.training_losses(model32, args[1], t, kwargs_of(args, T), noise=nz)
    o16 = tr16.diffusion.training_losses(model16, args[1], t, kwargs_of(args, T), noise=nz)
    assert torch.equal(o32["x_t"], o16["x_t"])                                     # the same kernel code on both sides: only eps differs
    c1, c2 = coefficients(tr32.diffusion, t)
    delta = (o16["pred"] - o32["pred"]).cpu()
    # the evaluation's own gate (test_gpu_eval.py: BF16_MAX / BF16_RMS against the reference) plus the fp32 side's distance from the reference
    A, R = BF16_MAX + FP32_ATOL, BF16_RMS + FP32_ATOL
    print(f"[losses bf16 {tag}] |eps16 - eps32| per row max {[f'{float(v):.2e}' for v in delta.abs().amax((1, 2))]} (gate {A:.2e}), "
          f"rms {float(delta.pow(2).mean().sqrt()):.2e} (gate {R:.2e})")
    assert float(delta.abs().max()) < A and float(delta.pow(2).mean().sqrt()) < R
    b = bounds(o32["pred"].cpu(), noise, o32["x_t"].cpu(), x0, c1, c2, A, float(f["huber_beta"]), R)
    check(f"bf16 {tag} mse", o16["mse"].cpu(), o32["mse"].cpu(), b["mse"])
    check(f"bf16 {tag} frame_mse", o16["frame_mse"].cpu(), o32["frame_mse"].cpu(), b["frame_mse"])
    for k in LR.SCALARS:
        check(f"bf16 {tag} {k}", o16["scalars"][k].cpu(), o32["scalars"][k].cpu(), b[k])


def test_loss_profile_levels_are_independent_and_nothing_syncs():
    cfg = get_config("show")
    model = gpu_model("show", "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B, T = 2, 24
    inp = make_inputs(cfg, B, frames=T, seed=61)
    x0 = torch.randn(B, T, cfg.net_dim_pose, generator=torch.Generator().manual_seed(62)).to(DEV)
    args = (inp["audio_emb"].to(DEV), x0, inp["person_id"].to(DEV), {"pretrain_aud_feat": inp["pretrain_aud_feat"].to(DEV)})
    calls = []
    orig = model.set_condition
    model.set_condition = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        torch.cuda.synchronize()
        checked = True
        try:
            torch.cuda.set_sync_debug_mode("error")
        except Exception as e:                                                  # this torch build has no sync debug mode: not checked
            checked = False
            print(f"[loss_profile] sync debug mode unavailable ({e}): host synchronisation inside the call is NOT checked")
        try:
            prof = tr.loss_profile(*args, levels=[0, 12, 24], seed=5)
        finally:
            if checked:
                torch.cuda.set_sync_debug_mode("default")
        print(f"[loss_profile] no blocking copy / synchronisation inside the call: {'checked' if checked else 'not checked'}")
        assert len(calls) == 1                                                     # the condition is set once for all levels
        one = tr.loss_profile(*args, levels=[12], seed=5)
        assert len(calls) == 1
    finally:
        del model.set_condition
    assert prof["levels"] == [0, 12, 24] and tuple(prof["mse"].shape) == (3, B) and tuple(prof["loss_model_pred"].shape) == (3,)
    assert prof["mse"].is_cuda and prof["mse"].dtype == torch.float64
    assert torch.equal(one["mse"][0], prof["mse"][1]) and torch.equal(one["xstart_mse"][0], prof["xstart_mse"][1])
    assert torch.equal(one["loss_model_pred"][0], prof["loss_model_pred"][1])
    ddim = tr.diffusion_ddim_val
    kw = kwargs_of(args, T)
    for i, k in enumerate([0, 12, 24]):
        out = ddim.training_losses(model, x0, k, kw, seed=level_seed(5, ddim.timestep_map[k]))
        assert torch.equal(out["mse"], prof["mse"][i]), k
        assert torch.equal(out["row_terms"][:, 2] / out["row_terms"][:, 5], prof["xstart_mse"][i])
        assert torch.equal(out["scalars"]["loss_model_pred"], prof["loss_model_pred"][i])
    assert not torch.equal(prof["mse"], tr.loss_profile(*args, levels=[0, 12, 24], seed=6)["mse"])
    # a timestep of the full process, addressed directly, is the level it is in the spaced one: same seed, same coefficients up to the tables
    full = tr.loss_profile(*args, levels=[480], seed=5, full=True)
    assert torch.allclose(full["mse"][0], prof["mse"][1], rtol=1e-4, atol=0)
    default = tr.loss_profile(*args, seed=5)
    assert default["levels"] == list(range(25)) and torch.equal(default["mse"][12], prof["mse"][1])
    print(f"[loss_profile] mse per level (clip 0): {[round(float(v), 4) for v in default['mse'][:, 0]]}")


def test_ragged_rows_equal_the_rows_alone():
    cfg = get_config("show")
    model = gpu_model("show", "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    diff = tr.diffusion
    B, T, lens, t = 2, 88, (20, 88), [500, 999]
    inp = make_inputs(cfg, B, frames=T, seed=71)
    x0 = torch.randn(B, T, cfg.net_dim_pose, generator=torch.Generator().manual_seed(72))
    noise = SeededNoise(73).randn((B, T, cfg.net_dim_pose))
    dev = {k: v.to(DEV) for k, v in inp.items()}
    args = (dev["audio_emb"], x0.to(DEV), dev["person_id"], {"pretrain_aud_feat": dev["pretrain_aud_feat"]})
    out = diff.training_losses(model, args[1], t, kwargs_of(args, T, torch.tensor(lens)), noise=noise.to(DEV))
    tl = tr.denoising_losses(*args, t=t, noise=noise.to(DEV), lengths=lens)
    assert torch.equal(tl["row_terms"], out["row_terms"])
    rows = out["row_terms"].cpu().numpy()
    assert np.array_equal(rows[:, 5], [n * cfg.net_dim_pose for n in lens]) and np.array_equal(rows[:, 6], [n - 1 for n in lens])
    assert not out["frame_mse"][0, 20:].any() and not out["pred_x0"][0, 20:].any() and not out["x_t"][0, 20:].any()
    assert bool((out["frame_mse"][0, :20] > 0).all()) and bool((out["frame_mse"][1] > 0).all())
    c1, c2 = coefficients(diff, t)
    beta = LR.HUBER_BETA
    for b, n in enumerate(lens):
        a_b = (args[0][b:b + 1, :n].contiguous(), args[1][b:b + 1, :n].contiguous(), args[2][b:b + 1],
               {"pretrain_aud_feat": args[3]["pretrain_aud_feat"][b:b + 1, :n].contiguous()})
        alone = diff.training_losses(model, a_b[1], t[b], kwargs_of(a_b, n), noise=noise[b:b + 1, :n].contiguous().to(DEV))
        assert torch.equal(alone["x_t"][0], out["x_t"][b, :n])
        eps_d = float((alone["pred"][0] - out["pred"][b, :n]).abs().max())
        # the existing gate on eps of a ragged row against the clip alone (tests/test_gpu_ragged.py: FP32_ATOL), through the sums
        A, k2 = FP32_ATOL, float(c2[b])
        p, nz, xt, x = (v[0].double().cpu().numpy() for v in (alone["pred"], alone["target"], alone["x_t"], alone["target_x0"]))
        d = np.abs(p - nz)
        xp = float(c1[b]) * xt - k2 * p
        dv = np.abs((xp[:-1] - xp[1:]) - (x[:-1] - x[1:]))
        split = cfg.split_pos
        bound = np.array([(2 * A * d[:, :split] + A * A).sum(), (2 * A * d[:, split:] + A * A).sum(),
                          (2 * k2 * A * np.abs(xp - x) + (k2 * A) ** 2).sum(), (4 * k2 * A * dv + (2 * k2 * A) ** 2).sum(), k2 * A / beta * d.size])
        want = alone["row_terms"][0].cpu().numpy()
        dist = np.abs(rows[b, :5] - want[:5])
        print(f"[losses ragged] row {b} ({n} frames): max |eps - eps alone| {eps_d:.3e}; row terms distance / gate "
              f"{[f'{v:.3f}' for v in dist / (bound + ROUND * np.abs(want[:5]))]}")
        assert eps_d < FP32_ATOL
        assert (dist <= bound + ROUND * np.abs(want[:5])).all() and np.array_equal(rows[b, 5:], want[5:])
    # Philox noise on a ragged batch: per-row streams, the bits q_sample draws itself
    keyed = diff.training_losses(model, args[1], t, kwargs_of(args, T, torch.tensor(lens)), seed=9, row_keys=[3, 4])
    assert torch.equal(keyed["x_t"], diff.q_sample(args[1], t, seed=9, row_keys=[3, 4], lengths=lens))
    with pytest.raises(ValueError, match="row_keys"):
        diff.training_losses(model, args[1], t, kwargs_of(args, T, torch.tensor(lens)), seed=9)
