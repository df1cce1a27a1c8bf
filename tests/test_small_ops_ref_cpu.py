"""The references of small_ops_ref.py without a GPU: the published Philox known answers, the moments of randn_ref, every reference inside
its own gate, and every listed mutant rejected on the very inputs the GPU tests (test_gpu_sampler_ops.py, test_gpu_row_ops.py) use - so
those inputs are shown to discriminate before a kernel ever sees them."""
import numpy as np
import pytest
import torch

import small_ops_ref as R


def test_philox_known_answers():
    for ctr, key, want in R.KNOWN_ANSWERS:
        got = R.philox4x32_10(ctr, key)
        assert [int(v) for v in got] == list(want), [hex(int(v)) for v in got]
    # vectorised: the three at once
    ctr = [np.array([k[0][i] for k in R.KNOWN_ANSWERS], dtype=np.uint32) for i in range(4)]
    key = [np.array([k[1][i] for k in R.KNOWN_ANSWERS], dtype=np.uint32) for i in range(2)]
    got = R.philox4x32_10(ctr, key)
    for j, (_, _, want) in enumerate(R.KNOWN_ANSWERS):
        assert [int(got[i][j]) for i in range(4)] == list(want)


def test_randn_ref_has_normal_moments():
    z = R.randn_ref(1 << 20, 42, 0)
    assert np.isfinite(z).all()
    assert abs(z.mean()) < 5e-3 and abs(z.std() - 1) < 5e-3
    assert abs((z ** 4).mean() - 3) < 0.05 and abs((z ** 3).mean()) < 0.02
    # cos and sin halves are uncorrelated
    assert abs(np.corrcoef(z[0::2], z[1::2])[0, 1]) < 5e-3


def test_philox_gate_calibration_and_float32_evaluation_passes():
    g = R.philox_gate_g()
    print(f"[philox] G (numpy float32 evaluation against the float64 reference, 2^20 counters, seed 42) = {g:.3f}")
    assert 0.5 < g < 4.0                      # a few ulp of r: 1.6 .. 1.7 where this was written
    for n, seed, off in R.PHILOX_CASES:
        z_ref, r_ref = R.randn_ref(n, seed, off, with_r=True)
        assert R.philox_ratio(R.randn_f32(n, seed, off), z_ref, r_ref) <= R.MARGIN * g


def _philox_inputs(mutant):
    """the GPU tests' launch a mutant must fail at"""
    keys, lens = list(R.PHILOX_ROW_KEYS), list(R.RAGGED_LENS)
    if mutant == "key_xor":
        return dict(n=len(keys) * 1028, seed=(0x1234 << 32) | 77, offset=3, row_keys=keys, n_row=1028)
    if mutant == "lens_ignored":
        return dict(n=len(keys) * R.RAGGED_T * 232, seed=42, offset=0, row_keys=keys, n_row=R.RAGGED_T * 232, row_lens=lens, draw=1, channels=232)
    return dict(n=1027, seed=42, offset=1)


@pytest.mark.parametrize("mutant", R.PHILOX_MUTANTS)
def test_philox_mutants_are_rejected(mutant):
    kw = _philox_inputs(mutant)
    z_ref, r_ref = R.randn_ref(with_r=True, **kw)
    ratio = R.philox_ratio(R.randn_ref(mutant=mutant, **kw), z_ref, r_ref)
    gate = R.MARGIN * R.philox_gate_g()
    print(f"[philox mutant] {mutant}: ratio {ratio:.3e} against the gate {gate:.2f}")
    assert ratio > 1e4 * gate
    # every case of the value test that can see the mutant at all rejects it too
    if "row_keys" not in kw:
        for n, seed, off in R.PHILOX_CASES:
            if mutant == "offset_elems" and off // 4 == off:
                continue
            zr, rr = R.randn_ref(n, seed, off, with_r=True)
            assert R.philox_ratio(R.randn_ref(n, seed, off, mutant=mutant), zr, rr) > gate, (n, seed, off)


def test_philox_stream_properties_hold_in_the_reference_and_fail_in_the_mutants():
    big = R.randn_ref(4 * 600 + 1027, 42, 0)
    assert np.array_equal(R.randn_ref(1027, 42, 600), big[2400:])
    assert not np.array_equal(R.randn_ref(1027, 42, 600, mutant="offset_elems"), big[2400:])
    a = R.randn_ref(64, 43, 0, row_keys=[0], n_row=64)
    b = R.randn_ref(64, 42, 0, row_keys=[1], n_row=64)
    assert not np.array_equal(a, b)
    assert np.array_equal(R.randn_ref(64, 43, 0, row_keys=[0], n_row=64, mutant="key_xor"), R.randn_ref(64, 42, 0, row_keys=[1], n_row=64, mutant="key_xor"))
    # ragged: row b is the solo stream of its own length
    keys, lens, Cc, T = list(R.PHILOX_ROW_KEYS), list(R.RAGGED_LENS), 192, R.RAGGED_T
    for draw in (0, 1, 5):
        z = R.randn_ref(4 * T * Cc, 42, 0, row_keys=keys, n_row=T * Cc, row_lens=lens, draw=draw, channels=Cc).reshape(4, -1)
        zm = R.randn_ref(4 * T * Cc, 42, 0, row_keys=keys, n_row=T * Cc, row_lens=lens, draw=draw, channels=Cc, mutant="lens_ignored").reshape(4, -1)
        for bi, (key, ln) in enumerate(zip(keys, lens)):
            m = ln * Cc
            solo = R.randn_ref(m, 42, draw * m // 4, row_keys=[key], n_row=m)
            assert np.array_equal(solo, z[bi, :m])
            assert np.array_equal(solo, zm[bi, :m]) == (draw == 0 or ln == T)


# ---- steps -----------------------------------------------------------------------------------------------------------------------------
def _ddim_buffers(t, L, combo, win, mutant=None):
    B, T, Cc = t["x"].shape
    prev = (t["x"], torch.full((B, T, Cc), R.SENTINEL), torch.full((B, L, Cc), R.SENTINEL))
    return R.ddim_expect(R.ddim_case_ref(t, L, combo, mutant if mutant and not mutant.startswith("window") else None), prev, win[0], win[1], mutant)


def _differs(a, b):
    return any(not torch.equal(x, y) for x, y in zip(a, b))


def _sees(mutant, combo):
    """only the combinations that exercise the mutated expression can tell it from the reference"""
    e, clip, mk, bl, tb, tails = combo
    return {"contract_noise1": R.ETA_MODES[e][2], "coef_is_s1m": e == "eta", "contract_gt": mk != "none" and not tails,
            "contract_fade": mk != "none" and bl, "linspace_one_sided": mk != "none" and bl, "clip_after_eps": clip,
            "tail_before_select": mk == "dense" and tails}.get(mutant, True)


@pytest.mark.parametrize("mutant", R.DDIM_MUTANTS)
def test_ddim_mutants_are_rejected_on_the_gpu_tests_inputs(mutant):
    wins = [w for w in R.STEP_WINDOWS if w[1] > w[0]] if mutant.startswith("window") else [R.STEP_WINDOWS[0]]
    for L in R.STEP_LS:
        t = R.step_inputs(L)
        for combo in R.step_combos():
            if not _sees(mutant, combo):
                continue
            for win in wins:
                if _differs(_ddim_buffers(t, L, combo, win, mutant), _ddim_buffers(t, L, combo, win)):
                    return                                    # the first case of the step test that tells the mutant from the reference
    raise AssertionError(f"no case of the step test tells {mutant} from the reference")


def test_ddim_reference_properties():
    L = 4
    t = R.step_inputs(L)
    # eta = 0 without the new fields is the expression the seam test already holds the kernel to
    from test_gpu_seam import _torch_ddim_step
    sc = R.ddim_scalars(1, 0.0)
    for mk in ("head", "dense"):
        for bl, tb in ((0, 0), (1, 0), (1, 1)):
            mine = R.ddim_step_ref(t["x"], t["eps"], sc, mask=t["masks"][mk], gt=t["gt"], nz2=t["nz2"], L=L, blend=bl, tail_blend=tb)[0]
            theirs = _torch_ddim_step(t["x"], t["eps"], t["gt"], t["masks"][mk], t["nz2"], sc[0], sc[1], sc[2], sc[3], L, bl, tb, 0, 0)
            assert torch.equal(mine, theirs)
    # the clamp bites on these inputs, sigma is positive at the eta level and zero at the last one
    x0 = R.ddim_step_ref(t["x"], t["eps"], sc)[1]
    assert float((x0.abs() > 1).float().mean()) > 0.05
    assert R.ddim_scalars(12, 0.5)[5] > 0 and R.ddim_scalars(0, 0.5)[5] == 0.0 and R.ddim_scalars(12, 0.5)[4] != R.ddim_scalars(12, 0.5)[3]
    # of the overlap lengths the step test uses, 4 is the one at which step * k and 1 - step * (L - 1 - k) differ in fp32
    assert [not torch.equal(R.linspace01(n, True), torch.linspace(0, 1, n)) for n in R.STEP_LS] == [False, False, True, False]


@pytest.mark.parametrize("mutant", R.DDPM_MUTANTS)
def test_ddpm_mutants_are_rejected(mutant):
    t = R.step_inputs(2)
    sc = R.ddpm_scalars(3)
    assert _differs(R.ddpm_step_ref(t["x"], t["eps"], t["nz1"], sc, 1, mutant), R.ddpm_step_ref(t["x"], t["eps"], t["nz1"], sc, 1))
    assert R.ddpm_scalars(0)[4] == 0.0 and sc[4] > 0


def test_undo_mutant_and_window_mutants_are_rejected():
    t = R.step_inputs(1)
    sc = R.undo_scalars(20)
    full = R.undo_step_ref(t["x"], t["nz1"], sc)
    assert not torch.equal(R.undo_step_ref(t["x"], t["nz1"], sc, "contract"), full)
    for (lo, hi) in R.STEP_WINDOWS[1:]:
        want = R.window(t["x"], full, lo, hi)
        assert not torch.equal(R.window(t["x"], full, lo + 1, hi), want) and not torch.equal(R.window(t["x"], full, lo, hi - 1), want)
        assert torch.equal(want[..., :lo], t["x"][..., :lo]) and torch.equal(want[..., hi:], t["x"][..., hi:])


# ---- temb, cfg_mix ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", R.TEMB_DIMS)
def test_temb_reference_gate_and_mutant(dim):
    t = list(R.TEMB_T)
    ref, allow = R.temb_ref64(t, dim), R.temb_allow(t, dim)
    e32 = (R.temb_f32(t, dim).double() - ref).abs()
    assert bool((e32 <= allow / R.MARGIN * (1 + 1e-12)).all()) and bool((e32[0] == 0).all())   # the calibration is the maximum over this population; t = 0 exact
    assert 0.5 < R.temb_k(dim) < 1.5                                            # torch's error is one rounding step of the scale's model
    assert float(allow[1:1000].max()) < 1e-3 and float(allow[1:8].max()) < 5e-6  # three digits and better up to t = 999, 2e-6 .. for the first steps
    bad = (R.temb_ref64(t, dim, "half_minus_1") - ref).abs()
    assert int((bad > allow).any(dim=1).sum()) == len(t) - 1                    # every row but t = 0
    # the embedding itself: cos | sin of t f_j with f_0 = 1
    assert torch.allclose(ref[:, 0], torch.cos(torch.tensor(t, dtype=torch.float64))) and torch.allclose(ref[:, dim // 2], torch.sin(torch.tensor(t, dtype=torch.float64)))


def test_cfg_mix_shortcut_mutant_is_rejected():
    for w in (103, 129):
        t = R.cfg_inputs(w, ld_extra=5, c0=3)
        e, x0 = R.cfg_mix_ref(t)
        em, x0m = R.cfg_mix_ref(t, mutant="no_shortcut")
        T = t["T"]
        assert torch.equal(e[:T], t["o"][t["cond_row0"]:t["cond_row0"] + T, :w])           # scale 1: o_c bit for bit
        assert not torch.equal(em[:T], e[:T]) and torch.equal(em[T:], e[T:])
        assert torch.equal(e[2 * T:], t["o"][2 * T:3 * T, :w])                               # scale 0: u + 0 (k - u) = u
        assert not torch.equal(x0m, x0)


# ---- data movement, FiLM ---------------------------------------------------------------------------------------------------------------
def test_im2col3_reference_against_unfold_and_lens():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 7, 5, generator=g)
    want = torch.nn.functional.unfold(torch.nn.functional.pad(x.transpose(1, 2), (1, 1))[:, :, None], (1, 3))       # [B, Cin * 3, T]
    want = want.view(3, 5, 3, 7).permute(0, 3, 2, 1).reshape(21, 15)
    assert torch.equal(R.im2col3_ref(x), want)
    lens = [7, 3, 0]
    got = R.im2col3_ref(x, lens).view(3, 7, 3, 5)
    for b, n in enumerate(lens):
        solo = R.im2col3_ref(x[b:b + 1, :n]).view(n, 3, 5) if n else None
        if n:
            assert torch.equal(got[b, :n], solo)
            assert bool((got[b, n + 1:] == 0).all()) and bool((got[b, n:, 1:] == 0).all())
        else:
            assert bool((got[b] == 0).all())


def test_film_fold_reference():
    t = R.film_inputs(3, 2, 128, ld_extra=8)
    A, Bc = R.film_fold_ref(t)
    r = t["tab"][:, :512].reshape(3, 2, 2, 128).double()
    assert torch.allclose(A.double(), t["gamma"][None].double() * (1 + r[:, :, 0]), rtol=3e-7, atol=0)
    want = t["beta"][None].double() * (1 + r[:, :, 0]) + r[:, :, 1]
    assert bool(((Bc.double() - want).abs() <= 2.0 ** -22 * (t["beta"].abs().max() * 5 + 5)).all())
    idx = [2, 2, 0, 1]
    A2, _ = R.film_fold_ref(t, idx)
    assert torch.equal(A2, A[idx])


# ---- LayerNorm family ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.LN_FAMILIES)
def test_ln_family_gates_accept_the_fp32_chain_and_reject_row_mixups(family):
    for kind, kw in (("pre", {}), ("film", {"frames": 26, "film_off": 8}), ("concat", {"widths": R.CONCAT_WIDTHS[2]})):
        M, D = 77, 999
        t = R.ln_inputs(kind, M, D, family, **kw)
        ref, allow, cal = R.ln_gate(t)
        assert 0 < cal < 1e-4 and bool((allow[:M] > 0).all())
        good = R._ln_chain(t, torch.float32, flip=True)[:M]
        assert R.ln_check(t, good, "chain32") <= R.MARGIN and R.ln_check(t, good.bfloat16(), "chain32 bf16") <= 1.0
        bad = dict(t)
        bad.pop("_gate")
        if kind == "pre":
            bad["X"] = t["h_in"]                                           # pre_add forgotten
        elif kind == "film":
            bad["clip"] = (t["clip"] + (torch.arange(t["X"].shape[0]) % 26 == 25)) % 3      # the last frame of a clip takes the next clip's row
        else:
            bad["X"] = t["X"].roll(1, dims=1)                              # segments off by one column
        with pytest.raises(AssertionError):
            R.ln_check(t, R._ln_chain(bad, torch.float32)[:M], "mutant")
    # pre: h + pre_add on the first n_pre rows only, in one fp32 add
    t = R.ln_inputs("pre", 5, 65, family)
    assert torch.equal(t["X"][:3], t["h_in"][:3] + t["pre_add"]) and torch.equal(t["X"][3:], t["h_in"][3:])
