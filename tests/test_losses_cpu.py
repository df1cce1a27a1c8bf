"""CPU tests (-m "not gpu") of the denoising losses: the float64 reference of the loss terms (tests/losses_ref.py) replays the three fixtures of
tests/golden/make_golden_losses.py from their stored model output and seeds — which pins the formulas, the two mirrored quirks of the
reference's backward_G included —, the uniform timestep sampler, the per-level seeds of loss_profile, and the refusals of training_losses /
denoising_losses, which come before any device call."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import losses_ref as LR
from diffsheg_amd import _lib
from diffsheg_amd.config import get_config
from diffsheg_amd.diffusion import (GaussianDiffusion, LossType, SpacedDiffusion, UniformSampler, create_named_schedule_sampler,
                                    space_timesteps)
from diffsheg_amd.model import UniDiffuser
from diffsheg_amd.synthetic import SeededNoise
from diffsheg_amd.trainer import DDPMTrainer, level_seed, sampler_namespace
from util import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["show", "show_cs1", "beat"]


def fixture_inputs(f):
    """x0, noise and the fp32 x_t / c1 / c2 of a loss fixture, rebuilt from its seeds exactly as the generator (and the reference's fp32
    q_sample: two rounded products and their rounded sum) made them."""
    cfg = get_config(str(f["dataset"]))
    B, T, C = int(f["batch"]), int(f["frames"]), cfg.net_dim_pose
    x0 = torch.randn(B, T, C, generator=torch.Generator().manual_seed(int(f["x0_seed"])))
    noise = SeededNoise(int(f["noise_seed"])).randn((B, T, C))
    diff = GaussianDiffusion(opt=sampler_namespace(cfg))
    t = [int(v) for v in f["t"]]
    a, s = diff.q_sample_coefficients(t, B)
    x_t = a.view(B, 1, 1) * x0 + s.view(B, 1, 1) * noise
    c1 = torch.from_numpy(diff.sqrt_recip_alphas_cumprod[t]).float()
    c2 = torch.from_numpy(diff.sqrt_recipm1_alphas_cumprod[t]).float()
    return cfg, x0, noise, x_t, c1, c2


@pytest.mark.parametrize("tag", CASES)
def test_reference_formulas_replay_the_fixture(tag):
    f = golden(f"losses_{tag}.npz")
    cfg, x0, noise, x_t, c1, c2 = fixture_inputs(f)
    assert [int(v) for v in f["t"]] == [0, 500, 999]                       # both ends and the middle of the process
    assert float(c1[2]) > 150                                              # t = 999: c1 = 1 / sqrt(alphas_cumprod) ~ 158
    beta = float(f["huber_beta"])
    assert beta == LR.HUBER_BETA
    pred = torch.from_numpy(f["pred"])
    rows = LR.row_terms_f64(pred, noise, x_t, x0, c1, c2, cfg.split_pos, beta)
    T, C = int(f["frames"]), cfg.net_dim_pose
    assert np.array_equal(rows[:, 5], np.full(3, T * C)) and np.array_equal(rows[:, 6], np.full(3, T - 1))
    mse = (rows[:, 0] + rows[:, 1]) / rows[:, 5]
    sc = LR.scalars_f64(rows, C, beta)
    worst = float(np.abs(mse / f["mse"] - 1).max())
    worst = max(worst, float(np.abs(LR.frame_mse_f64(pred, noise) / f["frame_mse"] - 1).max()))
    for k in LR.SCALARS:
        worst = max(worst, abs(sc[k] / float(f[k]) - 1))
    print(f"[losses {tag}] float64 replay against the fixture: worst relative difference {worst:.2e}")
    assert worst < 1e-12
    # the quirks, stated once more on the numbers: the unscaled velocity term, and no expression weight
    assert abs(sc["final_loss"] - (sc["loss_model_pred"] + sc["loss_vel_rec"] / 100 + sc["loss_x0_rec"])) < 1e-9 * sc["final_loss"]
    assert abs(sc["loss_model_pred"] - 1000 * (rows[:, 0] + rows[:, 1]).sum() / (3 * T * C)) < 1e-9 * sc["loss_model_pred"]


def test_reference_terms_are_ragged_row_by_row():
    g = torch.Generator().manual_seed(7)
    e, n, xt, x0 = (torch.randn(3, 11, 5, generator=g) for _ in range(4))
    c1, c2 = torch.tensor([1.0, 1.5, 158.0]), torch.tensor([0.1, 1.1, 158.0])
    lens = (1, 5, 11)
    rows = LR.row_terms_f64(e, n, xt, x0, c1, c2, 2, lens=lens)
    for b, L in enumerate(lens):
        alone = LR.row_terms_f64(e[b:b + 1, :L], n[b:b + 1, :L], xt[b:b + 1, :L], x0[b:b + 1, :L], c1[b:b + 1], c2[b:b + 1], 2)
        assert np.array_equal(rows[b], alone[0])
    assert rows[0, 3] == 0 and rows[0, 6] == 0                             # one frame: no pair
    assert np.array_equal(LR.frame_mse_f64(e, n, lens)[0, 1:], np.zeros(10))
    f32 = LR.row_terms_f32(e, n, xt, x0, c1, c2, 2, lens=lens)
    assert np.abs(f32[:, :5] - rows[:, :5]).max() <= 1e-4 * np.abs(rows[:, :5]).max()


def test_uniform_sampler_is_deterministic_and_in_range():
    cfg = get_config("show")
    full = GaussianDiffusion(opt=sampler_namespace(cfg))
    ddim = SpacedDiffusion(use_timesteps=space_timesteps(1000, "ddim25"), opt=sampler_namespace(cfg))
    for diff, n in ((full, 1000), (ddim, 25)):
        s = create_named_schedule_sampler("uniform", diff)
        assert isinstance(s, UniformSampler) and s.weights().shape == (n,)
        t1, w1 = s.sample(4096, "cpu", np.random.RandomState(5))
        t2, w2 = s.sample(4096, "cpu", np.random.RandomState(5))
        t3, _ = s.sample(4096, "cpu", np.random.RandomState(6))
        assert t1.dtype == torch.int64 and w1.dtype == torch.float32
        assert torch.equal(t1, t2) and torch.equal(w1, w2) and not torch.equal(t1, t3)
        assert int(t1.min()) >= 0 and int(t1.max()) < n and torch.equal(w1, torch.ones(4096))
        assert len(set(t1.tolist())) > n // 2                                # spread over the range, not stuck on a few values
    np.random.seed(11)
    a, _ = UniformSampler(full).sample(8, "cpu")                             # no generator: numpy's global state, as the reference
    np.random.seed(11)
    b, _ = UniformSampler(full).sample(8, "cpu")
    assert torch.equal(a, b)
    with pytest.raises(NotImplementedError):
        create_named_schedule_sampler("loss-second-moment", full)


def test_level_seed_depends_on_the_pair_alone():
    seeds = {t: level_seed(9, t) for t in range(0, 1000, 40)}
    assert len(set(seeds.values())) == len(seeds)
    assert level_seed(9, 480) == seeds[480] and level_seed(10, 480) != seeds[480]
    assert all(0 <= v < 1 << 64 for v in seeds.values())
    # loss_profile derives a level's seed from (seed, ORIGINAL timestep) and nothing else: the level list does not enter
    src = inspect.getsource(DDPMTrainer.loss_profile)
    assert "level_seed(seed, diff.timestep_map[k])" in src
    ddim = SpacedDiffusion(use_timesteps=space_timesteps(1000, "ddim25"), opt=sampler_namespace(get_config("show")))
    assert ddim.timestep_map[12] == 480 and ddim.timestep_map[0] == 0 and ddim.timestep_map[24] == 960


def _stub_model(ds="show"):
    m = UniDiffuser.__new__(UniDiffuser)                # no device: every refusal below must come before the model is touched
    m.cfg = get_config(ds)
    m._h = None
    m.device = torch.device("cpu")
    return m


def test_refusals_come_before_any_device_call():
    cfg = get_config("show")
    opt = sampler_namespace(cfg)
    model = _stub_model()
    x = torch.zeros(2, 8, cfg.net_dim_pose)
    kw = {"audio_emb": torch.zeros(2, 8, cfg.audio_dim), "person_id": torch.zeros(2, cfg.style_dim), "add_cond": {}, "y": {"anything": 1}}
    for lt in (LossType.KL, LossType.RESCALED_KL):
        with pytest.raises(NotImplementedError, match="loss_type"):
            GaussianDiffusion(opt=opt, loss_type=lt).training_losses(model, x, 3, kw)
    diff = GaussianDiffusion(opt=opt, loss_type=LossType.MSE)
    with pytest.raises(NotImplementedError, match="modalit"):
        diff.training_losses(model, x, 3, dict(kw, modality="expression"))
    with pytest.raises(NotImplementedError, match="pre_seq"):
        diff.training_losses(model, x, 3, dict(kw, pre_seq=torch.zeros(2, 4, cfg.net_dim_pose)))
    with pytest.raises(_lib.DshError, match="GPU"):
        diff.training_losses(model, x, 3, kw)                                 # a CPU x_start
    with pytest.raises(TypeError):
        diff.training_losses(lambda *a, **k: None, x, 3, kw)
    with pytest.raises(ValueError):
        diff.training_losses(model, x[0], 3, kw)
    # the default loss_type of this package's trainers (None) takes the MSE branch: the refusal it reaches is the CPU tensor
    with pytest.raises(_lib.DshError, match="GPU"):
        GaussianDiffusion(opt=opt).training_losses(model, x, 3, kw)


def test_trainer_refuses_a_batch_without_a_frame_pair():
    cfg = get_config("show")
    tr = DDPMTrainer(sampler_namespace(cfg), _stub_model())
    a = torch.zeros(2, 1, cfg.audio_dim)
    with pytest.raises(ValueError, match="frame pair"):
        tr.denoising_losses(a, torch.zeros(2, 1, cfg.net_dim_pose), torch.zeros(2, cfg.style_dim), {}, t=3)
    a = torch.zeros(2, 8, cfg.audio_dim)
    with pytest.raises(ValueError, match="frame pair"):
        tr.denoising_losses(a, torch.zeros(2, 8, cfg.net_dim_pose), torch.zeros(2, cfg.style_dim), {}, t=3, lengths=(1, 1))
    with pytest.raises(ValueError, match="levels"):
        tr.loss_profile(a, torch.zeros(2, 8, cfg.net_dim_pose), torch.zeros(2, cfg.style_dim), {}, levels=[25])
    assert isinstance(tr.sampler, UniformSampler) and tr.sampler.diffusion is tr.diffusion


def test_abi_surface():
    header = open(os.path.join(ROOT, "include", "diffsheg_hip.h")).read()
    assert "int dsh_op_denoise_losses(" in header and "int64_t dsh_denoise_losses_result_bytes(int32_t B, int32_t T);" in header
    macros = dict(re.findall(r"#define \w+_LOSS_(HEADER|COLS) (\d+)", header))
    assert macros == {"HEADER": str(_lib.LOSS_HEADER), "COLS": str(_lib.LOSS_COLS)}
    assert _lib.LOSS_COLS == LR.LOSS_COLS
    L = _lib.lib()
    chunks = lambda T: (T + 7) // 8
    for B, T in ((1, 1), (3, 88), (950, 88), (5, 34)):
        assert L.dsh_denoise_losses_result_bytes(B, T) == 8 * (_lib.LOSS_HEADER + B * _lib.LOSS_COLS + B * chunks(T) * 5)
    assert L.dsh_denoise_losses_result_bytes(0, 8) == -1 and L.dsh_denoise_losses_result_bytes(2, 0) == -1
    makefile = open(os.path.join(ROOT, "diffsheg_amd", "csrc", "Makefile")).read()
    assert "losses.hip" in makefile
