"""Few-step sampling, host side (no GPU): tables of a free timestep subset against the reference's SpacedDiffusion, the subset rules of
space_timesteps, the DPM-Solver++(2M) coefficients, the out-painting start level, the draw / step counts, and the solver's order on a
problem with a closed-form answer."""
import ctypes as C

import numpy as np
import pytest

import fewstep_ref as F
from diffsheg_amd import _lib
from diffsheg_amd.diffusion import (SpacedDiffusion, diffusion_table, diffusion_table_subset, masked_start_level, solver_coeffs,
                                    space_timesteps)
from oracle import sampler_ref as S
from util import golden

NAMES = ["betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
         "posterior_variance", "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2"]
SPECS = {"s10": "10", "s433": "4,3,3", "ddim10": "ddim10", "logsnr8": "logsnr8"}


def _opts(resp, kind=0, jl=3, jn=5, eta=0.0, son=0):
    return _lib.SamplerOptsC(kind, 1000, resp, jl, jn, 10, 1, 0, 0, 0, 0, 0, son, 0, eta)


def _arr(kept):
    return (C.c_int32 * max(len(kept), 1))(*kept), len(kept)


def test_subset_tables_match_the_reference_fixture():
    f = golden("fewstep_tables.npz")
    for tag, spec in SPECS.items():
        kept = sorted(space_timesteps(1000, spec))
        assert kept == [int(v) for v in f[f"{tag}__timestep_map"]], tag
        for n in NAMES:
            np.testing.assert_allclose(diffusion_table_subset(1000, kept, n), f[f"{tag}__{n}"], rtol=1e-15, atol=0, err_msg=f"{tag} {n}")
        # the oracle's tables of a kept list are pinned by the same fixture (the GPU tests replay loops on them)
        tb, _ = F.kept_tables(1000, kept)
        for n in NAMES:
            np.testing.assert_allclose(tb[n], f[f"{tag}__{n}"], rtol=1e-15, atol=0, err_msg=f"oracle {tag} {n}")


def test_stride_through_the_subset_form_is_bit_equal():
    for K in (25, 10, 3):
        kept = sorted(space_timesteps(1000, f"ddim{K}"))
        for n in NAMES + ["alphas_cumprod_next"]:
            a, b = diffusion_table_subset(1000, kept, n), diffusion_table(1000, K, n)
            assert a.tobytes() == b.tobytes(), (K, n)


def test_space_timesteps_rules():
    assert sorted(space_timesteps(1000, "logsnr8")) == F.LOGSNR8 == F.logsnr_timesteps(1000, 8)
    assert sorted(space_timesteps(1000, "logsnr10")) == F.LOGSNR10 == F.logsnr_timesteps(1000, 10)
    with pytest.raises(ValueError, match="39 distinct"):
        space_timesteps(1000, "logsnr40")
    assert space_timesteps(1000, "ddim25") == set(range(0, 1000, 40))
    for spec in ("10", "4,3,3", [4, 3, 3], "25", "1,1", [100, 0, 7]):
        counts = [int(v) for v in spec.split(",")] if isinstance(spec, str) else spec
        assert sorted(space_timesteps(1000, spec)) == F.section_timesteps(1000, counts), spec
    with pytest.raises(ValueError, match="cannot divide section of 333 steps into 334"):
        space_timesteps(1000, "10,10,334")
    with pytest.raises(ValueError):
        space_timesteps(1000, "a,b")


def test_spaced_diffusion_accepts_any_subset():
    kw = dict(opt=None, betas=diffusion_table(1000, 0, "betas"))
    d = SpacedDiffusion(use_timesteps=F.LOGSNR8, **kw)
    assert d._kept == F.LOGSNR8 and d.num_timesteps == 8 and d.timestep_map == F.LOGSNR8 and d.solver == "ddim"
    # (the respaced product of the new betas re-rounds the kept cumulative alphas: a few ulp, as in the reference)
    np.testing.assert_allclose(d.alphas_cumprod, diffusion_table(1000, 0, "alphas_cumprod")[F.LOGSNR8], rtol=1e-14, atol=0)
    s = SpacedDiffusion(use_timesteps=space_timesteps(1000, "ddim25"), **kw)
    assert s._kept is None and s.num_timesteps == 25                   # a stride takes the stride's own route
    assert s.alphas_cumprod.tobytes() == diffusion_table(1000, 25, "alphas_cumprod").tobytes()
    assert SpacedDiffusion(use_timesteps={3, 500, 998}, **kw)._kept == [3, 500, 998]     # (no integer stride gives these)
    for bad in (set(), {-1, 5}, {5, 1000}):
        with pytest.raises(ValueError):
            SpacedDiffusion(use_timesteps=bad, **kw)
    with pytest.raises(ValueError, match="solver"):
        SpacedDiffusion(use_timesteps=F.LOGSNR8, solver="heun", **kw)


def test_malformed_subsets_are_refused_by_the_table_entry():
    lib = _lib.lib()
    buf = (C.c_double * 8)()
    for bad, msg in (([5, 5, 9], b"ascending"), ([9, 5], b"ascending"), ([0, 1000], b"outside"), ([-1, 4], b"outside")):
        a, n = _arr(bad)
        assert lib.dsh_diffusion_table_subset(1000, a, n, b"betas", buf, 8) < 0 and msg in lib.dsh_last_error(), bad
    a, n = _arr([1, 2])
    assert lib.dsh_diffusion_table_subset(1000, a, 0, b"betas", buf, 8) < 0
    assert lib.dsh_solver_coeffs(1000, a, n, 2, (C.c_double * 3)()) < 0 and b"level" in lib.dsh_last_error()


def test_solver_coeffs_match_the_float64_restatement():
    for kept in (F.LOGSNR8, F.LOGSNR10, S.ddim_timestep_map(1000, "ddim25"), [3, 500, 998]):
        tb, _ = F.kept_tables(1000, kept)
        for k in range(len(kept)):
            got, want = solver_coeffs(1000, kept, k), F.solver_coeffs64(tb, k)
            for g, w, name in zip(got, want, "A Bc G".split()):
                assert abs(g - w) <= 1e-12 * abs(w), (kept[:3], k, name, g, w)
        assert solver_coeffs(1000, kept, 0) == (0.0, 1.0, 0.0)          # h is infinite at the last step: no second-order form
        assert solver_coeffs(1000, kept, len(kept) - 1)[2] == 0.0


def test_masked_start_level_and_schedules():
    lib = _lib.lib()
    assert masked_start_level(1000, F.LOGSNR10) == F.masked_start_level(1000, F.LOGSNR10) == 7
    assert masked_start_level(1000, F.LOGSNR8) == F.masked_start_level(1000, F.LOGSNR8)
    # the threshold is level 14 of the ddim25 table of the same process, 0.040879
    assert abs(diffusion_table(1000, 25, "alphas_cumprod")[14] - 0.040879) < 5e-7
    for K in (25, 10):                                                  # strides keep the reference's index rule
        kept = sorted(space_timesteps(1000, f"ddim{K}"))
        assert masked_start_level(1000, kept) == 0
        a, n = _arr(kept)
        o = _opts(K)
        for masked in (0, 1):
            assert lib.dsh_sample_num_steps_subset(C.byref(o), masked, 0, 0, a, n) == lib.dsh_sample_num_steps_from(C.byref(o), masked, 0, 0)
            assert lib.dsh_sample_num_draws_subset(C.byref(o), masked, 0, 0, a, n) == lib.dsh_sample_num_draws_from(C.byref(o), masked, 0, 0)
    o25 = _opts(25)
    assert lib.dsh_sample_num_steps_from(C.byref(o25), 1, 0, 0) == 63 + 48
    a, n = _arr(F.LOGSNR10)
    o = _opts(10)
    times = F.jump_schedule_from(7, 3, 5)
    evals = sum(1 for x, y in zip(times[:-1], times[1:]) if y < x)
    assert (evals, len(times) - 1 - evals) == (31, 24)
    assert lib.dsh_sample_num_steps_subset(C.byref(o), 1, 0, 0, a, n) == 55
    assert lib.dsh_sample_num_draws_subset(C.byref(o), 1, 0, 0, a, n) == 1 + 2 * 31 + 24
    assert lib.dsh_sample_num_steps_subset(C.byref(o), 0, 0, 0, a, n) == 10
    assert lib.dsh_sample_num_draws_subset(C.byref(o), 0, 0, 0, a, n) == 11
    # an explicit start level overrides the rule
    assert lib.dsh_sample_num_steps_subset(C.byref(o), 1, 1, 4, a, n) == len(F.jump_schedule_from(4, 3, 5)) - 1
    # refusals of the counting entries: another length, a DDPM loop
    assert lib.dsh_sample_num_steps_subset(C.byref(o), 0, 0, 0, a, 9) < 0 and b"respacing" in lib.dsh_last_error()
    assert lib.dsh_sample_num_draws_subset(C.byref(_opts(10, kind=1)), 0, 0, 0, a, n) < 0 and b"DDIM" in lib.dsh_last_error()


def test_second_order_on_a_problem_with_a_closed_form_answer():
    """Analytic denoiser for data ~ N(0, s^2): the figures of DESIGN.md 4.18.  The restatement alone gives ratios >= 6.5."""
    d25 = S.ddim_timestep_map(1000, "ddim25")
    for s in (0.5, 1.0):
        for N, kept in ((8, F.LOGSNR8), (10, F.LOGSNR10)):
            e1, e2 = F.analytic_errors(kept, s, "ddim"), F.analytic_errors(kept, s, "dpm2m")
            print(f"[analytic] s {s} logsnr{N}: ddim {e1:.3e} dpm2m {e2:.3e} ratio {e1 / e2:.2f}")
            assert e1 / e2 >= 4.0, (s, N, e1, e2)
        e25, e8 = F.analytic_errors(d25, s, "ddim"), F.analytic_errors(F.LOGSNR8, s, "dpm2m")
        print(f"[analytic] s {s}: ddim25 {e25:.3e}, logsnr8 dpm2m {e8:.3e}, {e25 / e8:.2f} x")
        if s == 0.5:
            assert e8 <= e25 / 3.0
    # the same loop with the library's own coefficients in place of the restatement's
    for kept in (F.LOGSNR8, F.LOGSNR10):
        tb, _ = F.kept_tables(1000, kept)
        ac, acp = tb["alphas_cumprod"], tb["alphas_cumprod_prev"]
        x, x0p, K, s = 1.0, None, len(kept), 0.5
        for k in range(K - 1, -1, -1):
            eps = np.sqrt(1 - ac[k]) * x / (ac[k] * s * s + 1 - ac[k])
            x0 = (x - np.sqrt(1 - ac[k]) * eps) / np.sqrt(ac[k])
            if k != 0 and k != K - 1:
                A, Bc, Gc = solver_coeffs(1000, kept, k)
                x = A * x + Bc * (x0 + Gc * (x0 - x0p))
            else:
                x = np.sqrt(acp[k]) * x0 + np.sqrt(1 - acp[k]) * eps
            x0p = x0
        err = abs(x - np.sqrt(s * s / (ac[K - 1] * s * s + 1 - ac[K - 1])))
        assert F.analytic_errors(kept, s, "ddim") / err >= 4.0
    # K <= 2: no step qualifies, the two solvers are one loop
    for kept in ([10, 900], [0, 999]):
        assert F.analytic_errors(kept, 0.5, "ddim") == F.analytic_errors(kept, 0.5, "dpm2m")
