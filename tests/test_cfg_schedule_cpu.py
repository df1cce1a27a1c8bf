"""Guidance schedules, host side (no GPU): the reference emulation of the scheduled mix against small_ops_ref.cfg_mix_ref, the mutants the
GPU gates (bit equality without rescale, 2 fp32 ulp with it) must reject on the very inputs the GPU tests use, and glue.CFGSchedule's
constructors and argument errors."""
import types

import numpy as np
import pytest
import torch

import cfg_schedule_ref as S
import fewstep_ref as F
import small_ops_ref as R
from diffsheg_amd.diffusion import space_timesteps
from diffsheg_amd.glue import CFGSchedule


# ---- the emulation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 103, 129])
def test_gain_one_is_the_plain_mix(w):
    ones = torch.ones(2, 7)
    for frames in (1, 5):
        for phi in (0.0,):
            t = S.sched_inputs(w, frames, (1.0, 1.15, 0.0), (0, 3, 6), table=ones, phi=phi)
            e, x0, f = S.cfg_mix_sched_ref(t)
            e0, x00 = R.cfg_mix_ref(t)
            assert torch.equal(e, e0) and torch.equal(x0, x00) and bool((f == 1).all())


def test_effective_scale_values():
    s = torch.tensor([2.0, 2.0, 2.0, 1.25, 0.0, 1.0], dtype=torch.float32)
    g = torch.tensor([0.5, 0.0, 1.0, 2.5, -1.0, 2.5], dtype=torch.float32)
    assert S.s_eff_ref(s, g).tolist() == [1.5, 1.0, 2.0, 1.625, 2.0, 1.0]
    # out-of-table timesteps read the nearest entry
    t = S.sched_inputs(5, 2, (2.0, 2.0, 2.0), (-3, 99, 2))
    lo = S.sched_inputs(5, 2, (2.0, 2.0, 2.0), (0, 6, 2))
    assert torch.equal(S.cfg_mix_sched_ref(t)[0], S.cfg_mix_sched_ref(lo)[0])


def test_pair_cases_cover_every_gain_and_scale():
    seen = {(s, float(S.TABLE[0][t])) for sc, ts in S.pair_cases() for s, t in zip(sc, ts)}
    assert seen == {(s, g) for s in S.SCALES for g in S.GAINS}
    assert tuple(S.TABLE[0][:5].tolist()) == S.GAINS


def _differs(t, mutant, what):
    """the mutant moves some valid element by more than the GPU gate allows (no rescale: any bit; rescale: more than 2 ulp)"""
    e, x0, _ = S.cfg_mix_sched_ref(t)
    em, x0m, _ = S.cfg_mix_sched_ref(t, mutant)
    v = S.valid_mask(t)
    a, b = (e, em) if what == "eps" else (x0, x0m)
    if t["phi"] > 0:
        return int(S.ulp_distance(a[v], b[v]).max()) > 2
    return not torch.equal(a[v], b[v])


def test_mutant_gain_applied_to_the_scale_is_rejected():
    hit = 0
    for sc, ts in S.pair_cases():
        for w in (1, 103, 129):
            hit += _differs(S.sched_inputs(w, 5, sc, ts), "gain_on_s", "eps")
    assert hit >= 3 * (len(S.pair_cases()) - 1)          # (1 + g (s - 1) = g s only where g = 1: nearly every case holds another gain)


def test_mutant_without_the_gain_shortcut_is_rejected():
    s = np.float32(0.15)
    assert np.float32(1.0) + (s - np.float32(1.0)) != s                       # 1 + (s - 1) is not s in fp32: the shortcut is observable
    t = S.sched_inputs(103, 5, (0.15, 0.15, 0.15), (1, 1, 1))                  # gain 1 for every clip
    assert _differs(t, "no_gain_shortcut", "eps")
    for s_exact in (1.25, 2.0):                                                # ... and not where the subtraction is exact
        assert not _differs(S.sched_inputs(103, 5, (s_exact,) * 3, (1, 1, 1)), "no_gain_shortcut", "eps")


@pytest.mark.parametrize("phi", [0.7, 1.0])
def test_rescale_mutants_are_rejected(phi):
    for w in (103, 129):
        t = S.sched_inputs(w, 5, (2.0, 2.0, 1.25), (1, 2, 3), phi=phi, lens=[5, 1, 3], ld_extra=40)
        _, _, f = S.cfg_mix_sched_ref(t)
        assert all(0.3 < v < 1.0 for v in f), f                                 # guidance blew the std up; the factor pulls it back
        assert _differs(t, "stats_padded", "eps")
        assert _differs(t, "stats_all_channels", "eps")
        assert _differs(t, "x0_unrescaled", "x0") and not _differs(t, "x0_unrescaled", "eps")
        # what the padded frames hold never reaches a valid element
        t2 = dict(t, o=t["o"].clone())
        for b, n in enumerate(t["lens"]):
            for half in (0, t["cond_row0"]):
                t2["o"][half + b * 5 + n:half + (b + 1) * 5] = float("nan")
        v = S.valid_mask(t)
        e, x0, f1 = S.cfg_mix_sched_ref(t)
        e2, x02, f2 = S.cfg_mix_sched_ref(t2)
        assert torch.equal(e[v], e2[v]) and torch.equal(x0[v], x02[v]) and np.array_equal(f1, f2)


def test_rescale_exact_cases():
    # n = 1: one frame of one column
    t = S.sched_inputs(1, 1, (2.0, 2.0, 2.0), (1, 1, 1), phi=1.0)
    assert bool((S.cfg_mix_sched_ref(t)[2] == 1).all())
    # a clip whose guided prediction is constant: sigma_e = 0
    t = S.sched_inputs(103, 5, (2.0, 2.0, 2.0), (1, 1, 1), phi=0.7)
    t["o"][0:5] = 0.25
    t["o"][t["cond_row0"]:t["cond_row0"] + 5] = 0.75
    e, _, f = S.cfg_mix_sched_ref(t)
    assert f[0] == 1 and bool((e[:5] == 1.25).all()) and f[1] != 1
    # s_eff = 1 (gain 0): k itself, whatever phi
    t = S.sched_inputs(103, 5, (2.0, 2.0, 2.0), (0, 1, 1), phi=1.0)
    e, _, f = S.cfg_mix_sched_ref(t)
    assert f[0] == 1 and torch.equal(e[:5], t["o"][t["cond_row0"]:t["cond_row0"] + 5, :103])
    # phi = 1 gives the guided prediction the conditional one's std (to the rounding of f and of the products)
    k = t["o"][t["cond_row0"] + 5:t["cond_row0"] + 10, :103].double().numpy()
    assert abs(np.std(e[5:10].double().numpy(), ddof=1) / np.std(k, ddof=1) - 1) < 1e-6


def test_ulp_distance():
    a = torch.tensor([1.0, -1.0, 0.0, 1e-3], dtype=torch.float32)
    b = torch.tensor(np.nextafter(a.numpy(), np.float32(2.0)))
    assert S.ulp_distance(a, b).tolist() == [1, 1, 1, 1] and S.ulp_distance(a, a).tolist() == [0, 0, 0, 0]
    assert int(S.ulp_distance(torch.tensor([-0.0]), torch.tensor([0.0]))[0]) == 0


# ---- glue.CFGSchedule --------------------------------------------------------------------------------------------------------------------
def test_defaults_floats_arrays_and_callables():
    s = CFGSchedule()
    assert s.steps == 1000 and s.trivial and s.same_for_both and s.rescale == (0.0, 0.0)
    assert s.expression.dtype == np.float32 and s.expression.shape == (1000,) and bool((s.gesture == 1).all())
    s = CFGSchedule(expression=0.5, gesture=lambda t: 1.0 if t < 400 else 0.0, rescale=(0.7, 0.3))
    assert bool((s.expression == 0.5).all()) and s.gesture[399] == 1 and s.gesture[400] == 0
    assert s.rescale == (float(np.float32(0.7)), float(np.float32(0.3))) and not s.trivial and not s.same_for_both
    ramp = np.linspace(0, 2, 10)
    s = CFGSchedule(ramp, torch.tensor(ramp), steps=10, rescale=1)
    assert np.array_equal(s.expression, ramp.astype(np.float32)) and s.same_for_both and s.rescale == (1.0, 1.0)
    assert CFGSchedule(0.5) == CFGSchedule(np.full(1000, 0.5)) and CFGSchedule(0.5) != CFGSchedule(0.5, rescale=0.1)
    assert CFGSchedule(rescale=0.2) != CFGSchedule() and not CFGSchedule(rescale=0.2).trivial


def test_interval_against_a_hand_written_table():
    s = CFGSchedule.interval(200, 599, rescale=0.5)
    want = np.array([1.0 if 200 <= t <= 599 else 0.0 for t in range(1000)], dtype=np.float32)
    assert np.array_equal(s.expression, want) and np.array_equal(s.gesture, want) and s.rescale == (0.5, 0.5)
    s = CFGSchedule.interval(0, 3, steps=5)
    assert s.expression.tolist() == [1, 1, 1, 1, 0]
    for lo, hi in ((-1, 5), (7, 3), (0, 1000)):
        with pytest.raises(ValueError, match="interval"):
            CFGSchedule.interval(lo, hi)


def _diffusion(spec):
    return types.SimpleNamespace(timestep_map=sorted(space_timesteps(1000, spec)), original_num_steps=1000)


def test_from_levels_ddim25():
    d = _diffusion("ddim25")
    assert d.timestep_map == list(range(0, 1000, 40))
    gains = [0.1 * k for k in range(25)]
    s = CFGSchedule.from_levels(d, gains, rescale=0.7)
    # a timestep takes the gain of the smallest kept timestep >= it: t = 0 -> level 0, 1 .. 40 -> level 1, ..., 921 .. 999 -> level 24
    want = np.array([gains[min((t + 39) // 40, 24)] for t in range(1000)], dtype=np.float32)
    assert np.array_equal(s.expression, want) and np.array_equal(s.gesture, want) and s.rescale[0] == float(np.float32(0.7))
    for k, t in enumerate(d.timestep_map):
        assert s.expression[t] == np.float32(gains[k])
    assert s.expression[41] == np.float32(gains[2]) and s.expression[999] == np.float32(gains[24])
    g2 = [1.0] * 25
    s = CFGSchedule.from_levels(d, gains, gesture_gains=g2)
    assert bool((s.gesture == 1).all()) and np.array_equal(s.expression, want)
    with pytest.raises(ValueError, match="one gain per level"):
        CFGSchedule.from_levels(d, gains[:24])


def test_from_levels_logsnr8():
    d = _diffusion("logsnr8")
    kept = F.LOGSNR8
    assert d.timestep_map == kept and len(kept) == 8
    gains = [0.0, 0.25, 0.5, 1.0, 1.0, 2.0, 0.5, 0.0]
    s = CFGSchedule.from_levels(d, gains)
    want = np.empty(1000, dtype=np.float32)
    for t in range(1000):
        above = [k for k, v in enumerate(kept) if v >= t]
        want[t] = gains[above[0] if above else 7]
    assert np.array_equal(s.expression, want)
    assert [float(s.expression[t]) for t in kept] == gains


def test_argument_errors():
    for bad in (float("nan"), float("inf"), [1.0] * 999, "x", 1e39):
        with pytest.raises(ValueError, match="CFGSchedule"):
            CFGSchedule(expression=bad)
    with pytest.raises(ValueError, match="finite"):
        CFGSchedule(gesture=lambda t: float("inf") if t == 7 else 1.0)
    for bad in (-0.1, 1.5, float("nan"), (0.1, 0.2, 0.3), (0.5, 2.0)):
        with pytest.raises(ValueError, match="rescale"):
            CFGSchedule(rescale=bad)
    for bad in (0, -5, 2.5):
        with pytest.raises(ValueError, match="steps"):
            CFGSchedule(steps=bad)
