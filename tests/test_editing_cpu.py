"""Editing an existing take, the host side: the alphas_cumprod_next table against the reference's, draw / step counts of the schedules
that start at a level against a Python restatement, the strength -> level mapping, every refusal (raised before anything reaches a
device) and the host validation of glue.edit_region."""
import ctypes as C

import numpy as np
import pytest
import torch

from diffsheg_amd import _lib, glue
from diffsheg_amd.config import get_config
from diffsheg_amd.diffusion import diffusion_table
from diffsheg_amd.model import UniDiffuser
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace
from util import golden

RESP = 25


def test_alphas_cumprod_next_matches_reference():
    ref = golden("edit_tables_ddim25.npz")["alphas_cumprod_next"]
    got = diffusion_table(1000, RESP, "alphas_cumprod_next")
    assert got.shape == ref.shape == (RESP,) and got.dtype == np.float64
    assert float(np.abs(got - ref).max()) <= 1e-15
    ac = diffusion_table(1000, RESP, "alphas_cumprod")
    assert np.array_equal(got[:-1], ac[1:]) and got[-1] == 0.0
    full = diffusion_table(1000, 0, "alphas_cumprod_next")
    assert full.shape == (1000,) and full[-1] == 0.0 and np.array_equal(full[:-1], diffusion_table(1000, 0, "alphas_cumprod")[1:])


# ---- counts ------------------------------------------------------------------------------------------------------------------
def _opts(**over):
    d = dict(kind=0, diffusion_steps=1000, respacing=RESP, jump_length=3, jump_n_sample=5, overlap_len=10, add_blend=1, no_resample=0,
             no_repaint=0, clip_denoised=0, noise_mode=1, seed=0, same_overlap_noisy=0, clip_idx=0, eta=0.0)
    d.update(over)
    return _lib.SamplerOptsC(*[d[n] for n, _ in _lib.SamplerOptsC._fields_])


def _walk(t_T, jl, jn):
    """the RePaint time list from t_T: one level down per step; the first jn - 1 arrivals at a level 0, jl, 2 jl, .. < t_T - jl go jl levels back up"""
    left = {j: jn - 1 for j in range(0, t_T - jl, jl)}
    t, ts = t_T, []
    while t >= 1:
        t -= 1
        ts.append(t)
        if left.get(t, 0) > 0:
            left[t] -= 1
            for _ in range(jl):
                t += 1
                ts.append(t)
    return ts + [-1]


def _expected(masked, init, K, jl=3, jn=5):
    """(draws, steps): a DDIM step takes its randn_like (and the noised gt's draw when masked), an undo step one draw; x_T / the q_sample noise one more"""
    first = 0 if init == 1 else 1
    if not masked:
        n = K if K else RESP
        return first + n, n
    ts = _walk(K if K else 15, jl, jn)
    den = sum(1 for a, b in zip(ts[:-1], ts[1:]) if b < a)
    undo = len(ts) - 1 - den
    return first + 2 * den + undo, den + undo


@pytest.mark.parametrize("masked", [0, 1])
@pytest.mark.parametrize("init", [0, 1, 2])
def test_counts_from_a_level_match_the_restatement(masked, init):
    lib = _lib.lib()
    o = _opts()
    for K in range(0, RESP + 1):
        want = _expected(masked, init, K)
        got = (lib.dsh_sample_num_draws_from(C.byref(o), masked, init, K), lib.dsh_sample_num_steps_from(C.byref(o), masked, init, K))
        assert got == want, (K, got, want)
    o2 = _opts(jump_length=2, jump_n_sample=3)
    for K in (1, 2, 3, 7, 25):
        want = _expected(masked, init, K, 2, 3)
        assert (lib.dsh_sample_num_draws_from(C.byref(o2), masked, init, K), lib.dsh_sample_num_steps_from(C.byref(o2), masked, init, K)) == want


def test_start_level_zero_equals_the_existing_entries():
    lib = _lib.lib()
    for o in (_opts(), _opts(no_resample=1), _opts(no_repaint=1), _opts(kind=1, respacing=1), _opts(respacing=20)):
        for masked in (0, 1):
            if o.kind == 1 and masked:
                continue
            assert lib.dsh_sample_num_steps_from(C.byref(o), masked, 0, 0) == lib.dsh_sample_num_steps(C.byref(o), masked) > 0
            for init in (0, 1):
                assert lib.dsh_sample_num_draws_from(C.byref(o), masked, init, 0) == lib.dsh_sample_num_draws(C.byref(o), masked, init) > 0
    o = _opts()
    assert (lib.dsh_sample_num_draws(C.byref(o), 0, 0), lib.dsh_sample_num_draws(C.byref(o), 1, 0), lib.dsh_sample_num_steps(C.byref(o), 1)) == (26, 175, 111)


def test_counts_refuse_what_the_loop_refuses():
    lib = _lib.lib()
    o = _opts()
    for bad in (-1, RESP + 1, 1000):
        assert lib.dsh_sample_num_steps_from(C.byref(o), 0, 0, bad) == -1
        assert lib.dsh_sample_num_draws_from(C.byref(o), 0, 2, bad) == -1
    assert lib.dsh_sample_num_draws_from(C.byref(o), 0, 3, 5) == -1
    ddpm = _opts(kind=1)
    assert lib.dsh_sample_num_steps_from(C.byref(ddpm), 0, 0, 5) == -1
    assert b"DDIM" in lib.dsh_last_error()
    assert lib.dsh_sample_num_draws_from(C.byref(ddpm), 0, 2, 0) == -1                   # "x holds x0" on a DDPM loop
    assert lib.dsh_sample_num_draws_from(C.byref(ddpm), 0, 1, 0) == 1000 and lib.dsh_sample_num_draws(C.byref(ddpm), 0, 2) == 1000


# ---- strength -> level, refusals -----------------------------------------------------------------------------------------------
def test_strength_maps_to_a_level():
    f = DDPMTrainer.strength_to_level
    assert [f(s) for s in (1.0, 0.4, 0.2, 0.04, 0.01, 1e-6, 0.98, 0.5)] == [25, 10, 5, 1, 1, 1, 24, 12]
    assert f(0.5, 20) == 10
    for bad in (0.0, -0.1, 1.0001, 2):
        with pytest.raises(ValueError):
            f(bad)


def _cpu_model():
    m = object.__new__(UniDiffuser)          # refusals come before anything of the model is touched
    m.device = torch.device("cpu")
    return m


def _trainer(**over):
    cfg = get_config("show")
    return cfg, DDPMTrainer(sampler_namespace(cfg, **over), _cpu_model())


def _kw(y=None):
    return {"audio_emb": None, "length": None, "person_id": None, "add_cond": {}, "y": {} if y is None else y, "pe_type": "pe_sinu"}


def test_loop_refusals():
    cfg, tr = _trainer()
    m, shape = tr.encoder, (1, cfg.n_poses, cfg.net_dim_pose)
    x = torch.zeros(shape)
    ddim, full = tr.diffusion_ddim_val, tr.diffusion
    with pytest.raises(TypeError):                       # DDPM loops
        full.p_sample_loop(m, shape, noise=x, model_kwargs=_kw(), start_level=5)
    with pytest.raises(TypeError):
        full.p_sample_loop(m, shape, model_kwargs=_kw(), x_start=x)
    for bad in (0, -3, RESP + 1):                        # out of range
        with pytest.raises(ValueError):
            ddim.ddim_sample_loop(m, shape, noise=x, model_kwargs=_kw(), start_level=bad)
    with pytest.raises(ValueError):                      # both
        ddim.ddim_sample_loop(m, shape, noise=x, x_start=x, model_kwargs=_kw(), start_level=5)
    with pytest.raises(ValueError):                      # neither
        ddim.ddim_sample_loop(m, shape, model_kwargs=_kw(), start_level=5)
    with pytest.raises(NotImplementedError):
        ddim.ddim_sample_loop(m, shape, noise=x, model_kwargs=_kw(), start_level=5, tail_blend=True)
    _, tr_son = _trainer(same_overlap_noisy=True)
    with pytest.raises(NotImplementedError):
        tr_son.diffusion_ddim_val.ddim_sample_loop(tr_son.encoder, shape, noise=x, model_kwargs=_kw({"clip_idx": 0}), start_level=5)


def test_reverse_loop_refusals():
    cfg, tr = _trainer()
    m = tr.encoder
    x = torch.zeros(1, cfg.n_poses, cfg.net_dim_pose)
    ddim = tr.diffusion_ddim_val
    with pytest.raises(ValueError):
        ddim.ddim_reverse_sample_loop(m, x, 5, model_kwargs=_kw(), eta=0.5)
    with pytest.raises(ValueError):
        ddim.ddim_reverse_sample(m, x, 3, model_kwargs=_kw(), eta=1.0)
    mask = torch.ones_like(x, dtype=torch.bool)
    with pytest.raises(NotImplementedError):
        ddim.ddim_reverse_sample_loop(m, x, 5, model_kwargs=_kw({"gt": x, "outpainting_mask": mask}))
    for bad in (0, -1, RESP + 1):
        with pytest.raises(ValueError):
            ddim.ddim_reverse_sample_loop(m, x, bad, model_kwargs=_kw())
    with pytest.raises(ValueError):
        ddim.ddim_reverse_sample(m, x, RESP, model_kwargs=_kw())
    with pytest.raises(NotImplementedError):
        tr.diffusion.ddim_reverse_sample_loop(m, x, 5, model_kwargs=_kw())          # not a SpacedDiffusion


def test_trainer_refusals():
    cfg, tr = _trainer()
    T, Cc = cfg.n_poses, cfg.net_dim_pose
    audio, pid, mot = torch.zeros(1, T, cfg.audio_dim), torch.zeros(1, cfg.style_dim), torch.zeros(1, T, Cc)
    for kw in ({}, {"level": 5, "strength": 0.5}, {"level": 0}, {"level": RESP + 1}, {"strength": 0.0}, {"strength": 1.5}):
        with pytest.raises(ValueError):
            tr.sample_variations(mot, audio, pid, {}, **kw)
    with pytest.raises(ValueError):
        tr.sample_variations(mot[:, :-1], audio, pid, {}, level=5)
    with pytest.raises(ValueError):
        tr.sample_variations(mot, audio, pid, {}, level=5, keep=torch.ones(1, T, Cc))           # not bool
    with pytest.raises(ValueError):
        tr.sample_variations(mot, audio, pid, {}, level=5, keep=torch.ones(2, 3, dtype=torch.bool))
    with pytest.raises(ValueError):
        tr.restyle(mot, audio, pid, pid, {}, level=0)
    _, tr_fhv = _trainer(fix_head_var=True)
    with pytest.raises(NotImplementedError):
        tr_fhv.sample_variations(mot, audio, pid, {}, level=5)
    _, tr_ddpm = _trainer(ddim=False)
    with pytest.raises(NotImplementedError):
        tr_ddpm.sample_variations(mot, audio, pid, {}, level=5)
    with pytest.raises(NotImplementedError):
        tr_ddpm.restyle(mot, audio, pid, pid, {}, level=5)


def test_q_sample_host_checks():
    cfg, tr = _trainer()
    d = tr.diffusion_ddim_val
    a, s = d.q_sample_coefficients(torch.tensor([0, 9, 24]), 3)
    ac = diffusion_table(1000, RESP, "alphas_cumprod")
    assert a.dtype == s.dtype == torch.float32
    assert np.array_equal(a.numpy(), np.sqrt(ac[[0, 9, 24]]).astype(np.float32))
    assert np.array_equal(s.numpy(), np.sqrt(1.0 - ac[[0, 9, 24]]).astype(np.float32))
    assert torch.equal(d.q_sample_coefficients(9, 2)[0], a[1:2].expand(2))
    for bad in (-1, RESP, [1, 2]):
        with pytest.raises(ValueError):
            d.q_sample_coefficients(bad, 3)
    with pytest.raises(_lib.DshError):
        d.q_sample(torch.zeros(1, 4, 4), 3)              # no CPU path
    _, tr_fhv = _trainer(fix_head_var=True)
    assert tr_fhv.diffusion_ddim_val._fixed_from() == 90 and d._fixed_from() == -1
    _, tr_b = _trainer(fix_head_var=True, dataset_name="freeform_all")
    assert tr_b.diffusion_ddim_val._fixed_from() == 24
    _, tr_x = _trainer(fix_head_var=True, dataset_name="beat")
    with pytest.raises(NotImplementedError):
        tr_x.diffusion_ddim_val.q_sample(torch.zeros(1, 4, 4), 3)


def test_edit_region_host_validation():
    for kw in ({"frames": [(-1, 4)]}, {"frames": [(5, 4)]}, {"frames": [(0, 9)]}, {"columns": [(0, 7)]}, {"columns": [(3, 2)]},
               {"frames": torch.tensor([[0, 4]])}, {"frames": torch.tensor([[0, 4], [2, 9]])}):
        with pytest.raises(ValueError):
            glue.edit_region(2, 8, 6, **kw)
    with pytest.raises(ValueError):
        glue.edit_region(0, 8, 6, frames=[(0, 1)])
    with pytest.raises(_lib.DshError):
        glue.edit_region(2, 8, 6, frames=[(0, 4)], device="cpu")      # valid ranges: the refusal left is the missing CPU path
