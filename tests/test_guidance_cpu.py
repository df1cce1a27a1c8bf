"""CPU tests (-m "not gpu") of the runtime guidance scale: the guidance fixtures (tests/golden/make_golden_guidance.py, the
imported reference at runtime values of opt.cond_scale) against the oracle at the same scales, which pins the fixtures the GPU
tests read; the host-side normalisation of a scale argument; the C declaration and its binding."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from diffsheg_amd import _lib
from diffsheg_amd.config import get_config
from diffsheg_amd.model import normalize_guidance_scale
from diffsheg_amd.synthetic import make_inputs
from oracle import denoiser_ref as D
from oracle import sampler_ref as S
from util import golden, synthetic_sd

torch.set_num_threads(min(8, os.cpu_count() or 1))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _eval_fixture_eps(f, tag, st):
    return np.concatenate([f[f"{tag}_{st}_eps_ges"], f[f"{tag}_{st}_eps_exp"]], axis=-1)


@pytest.mark.parametrize("st,scale", [("s100", 1.0), ("s115", 1.15), ("s200", 2.0)])
def test_guidance_eval_fixture_matches_oracle(st, scale):
    f = golden("guidance_show.npz")
    cfg = dataclasses.replace(get_config("show"), cond_scale=scale)
    assert float(f["scales"][["s100", "s115", "s200"].index(st)]) == scale
    sd = synthetic_sd("show")
    B = int(f["batch"])
    inp = make_inputs(cfg, B, seed=int(f["input_seed"]))
    for tag in ("k0", "k14"):
        t = torch.full((B,), int(f[f"{tag}_t"]))
        c1, c2 = torch.tensor(np.float32(f[f"{tag}_c1"])), torch.tensor(np.float32(f[f"{tag}_c2"]))
        with torch.no_grad():
            eps, parts = D.unidiffuser(sd, cfg, inp["x_T"], t, c1, c2, inp["audio_emb"], inp["person_id"],
                                       inp["pretrain_aud_feat"], return_parts=True)
        np.testing.assert_allclose(eps, _eval_fixture_eps(f, tag, st), atol=2e-6)
        np.testing.assert_allclose(parts["eps_exp"], f[f"{tag}_{st}_eps_exp"], atol=2e-6)


def test_guidance_eval_fixture_scales_differ():
    """The three scales give three different outputs (the fixture is not the same vector three times)."""
    f = golden("guidance_show.npz")
    a, b, c = (_eval_fixture_eps(f, "k14", st) for st in ("s100", "s115", "s200"))
    assert np.abs(a - b).max() > 1e-3 and np.abs(b - c).max() > 1e-3


def test_guidance_ddim_fixture_matches_oracle():
    f = golden("ddim25_guidance_show.npz")
    cfg = dataclasses.replace(get_config("show"), cond_scale=float(f["cond_scale"]))
    sd = synthetic_sd("show")
    B = int(f["batch"])
    inp = make_inputs(cfg, B, seed=int(f["input_seed"]))

    def eps_fn(x, t, c1, c2):
        with torch.no_grad():
            return D.unidiffuser(sd, cfg, x, torch.full((B,), t), c1, c2, inp["audio_emb"], inp["person_id"], inp["pretrain_aud_feat"])
    src = S.NoiseSource(seed=int(f["noise_seed"]))
    tr = []
    x = S.ddim_sample_loop(eps_fn, (B, cfg.n_poses, cfg.net_dim_pose), {}, src, trace=tr)
    assert src.i == int(f["draws"]) == 26
    for i, (_, k, xs, x0) in enumerate(tr):
        assert k == 24 - i
        np.testing.assert_allclose(xs[:, :3, :6], f["step_corner"][i], rtol=1e-6, atol=1e-6)
    scale = float(np.abs(f["final"]).max())
    assert float((x - torch.from_numpy(f["final"])).abs().max()) <= 1e-6 * scale


# ---- host-side argument normalisation ---------------------------------------------------------------------------------
def test_normalize_none_is_config_value():
    assert normalize_guidance_scale(None) is None


@pytest.mark.parametrize("arg", [1.15, 2, np.float32(1.15), np.array(1.15), torch.tensor(1.15), torch.tensor(1.15, dtype=torch.float64)])
def test_normalize_scalar_forms(arg):
    assert normalize_guidance_scale(arg) == (float(np.float32(1.15 if not isinstance(arg, int) else 2)),)


@pytest.mark.parametrize("arg", [[1.15, 2.0, 0.0], (1.15, 2.0, 0.0), np.array([1.15, 2.0, 0.0]), torch.tensor([1.15, 2.0, 0.0])])
def test_normalize_per_row_forms(arg):
    want = tuple(float(v) for v in np.array([1.15, 2.0, 0.0], dtype=np.float32))
    assert normalize_guidance_scale(arg) == want


def test_normalize_values_are_float32():
    """What the kernels read: 1.15 rounded to fp32, exactly 1 stays 1 (the rows that take k)."""
    (v,) = normalize_guidance_scale(1.15)
    assert v == float(np.float32(1.15)) and v != 1.15
    assert normalize_guidance_scale([1.0, 1]) == (1.0, 1.0)


@pytest.mark.parametrize("bad", [float("nan"), [1.0, float("inf")], torch.tensor([float("nan")]), 1e39, [], "1.15", [[1.0, 2.0]],
                                 torch.ones(2, 2)])
def test_normalize_rejects(bad):
    with pytest.raises(ValueError):
        normalize_guidance_scale(bad)


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_set_guidance_scale():
    hdr = open(os.path.join(ROOT, "include", "diffsheg_hip.h")).read()
    assert "int dsh_set_guidance_scale(dsh_ctx* ctx, const float* scales_host, int32_t n);" in hdr
    assert "dsh_set_guidance_scale" in _lib.SYMBOLS
