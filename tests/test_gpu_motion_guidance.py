"""Soft constraints while sampling on a real MI355X.

1. the native loops with a MotionGuidance(space="x_t") against the imported reference running the same object as its cond_fn
   (tests/golden/make_golden_motion_guidance.py), under the sampler's bar: REL_TOL of the reference's range per step and end to end;
2. the three op-level entries against the float64 restatement of tests/motion_guidance_ref.py, gated at 4 x the error of the same
   restatement run in fp32 torch on the CPU (the precedent of the rotation kernels);
3. invariances, bit for bit: batch, column range, the two-encoder pipeline, sub-batch streams, zero guidance;
4. the x0 space and the dpm2m solver end to end against a float64 replay of the loop driven by the device's own eps;
5. attraction brings the sample nearer its targets (checked on the CPU with the reference when the fixtures were made: it holds
   strictly for all four).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import motion_guidance_ref as R  # noqa: E402
from diffsheg_amd import _lib  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.diffusion import diffusion_table, diffusion_table_subset, logsnr_timesteps, solver_coeffs  # noqa: E402
from diffsheg_amd.glue import MotionGuidance  # noqa: E402
from diffsheg_amd.synthetic import SeededNoise, make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from test_gpu_sampler import REL_TOL, _check_trace, _kwargs, _masked, _sample_flags  # noqa: E402
from util import assert_split_ran, golden, gpu_model, rel_err  # noqa: E402

DEV = "cuda:0"
GATE = 4.0          # kernel error <= GATE x the error of the fp32 torch run of the same restatement (both against float64)


def _guidance(case, B, T, Cc, levels, space="x_t"):
    f = R.fixture_guidance(case, B, T, Cc, levels)
    dev = lambda v: None if v is None else v.to(DEV)
    return MotionGuidance(dev(f["target"]), dev(f["weight"]), dev(f["vel"]), dev(f["acc"]), space=space, level_scale=f["level_scale"]), f


# ---- 1. reference fixtures, 5. behaviour ------------------------------------------------------------------------------------------
CASES = {"plain": ("mguide_ddim25_plain_show.npz", "ddim25_plain_show.npz"), "harmonize": ("mguide_harmonize_show_3_2.npz", "ddim25_harmonize_show_3_2.npz"),
         "eta": ("mguide_ddim25_eta05_show.npz", "ddim25_eta05_show.npz"), "ddpm": ("mguide_ddpm50_beat.npz", None)}
_RUNS = {}


def _run_case(case):
    """One native run per fixture, shared by the parity test and the behaviour test: (x, trace, draws, fixture, guidance terms, the
    reference's unguided final sample of the same inputs)."""
    if case in _RUNS:
        return _RUNS[case]
    f = golden(CASES[case][0])
    base = torch.from_numpy(golden(CASES[case][1])["final"] if CASES[case][1] else f["final_unguided"])
    ds = "beat" if case == "ddpm" else "show"
    cfg = get_config(ds, jump_length=3, jump_n_sample=2) if case == "harmonize" else get_config(ds)
    model = gpu_model(ds, "fp32")
    B = int(f["batch"])
    shape = (B, cfg.n_poses, cfg.net_dim_pose)
    src = SeededNoise(int(f["noise_seed"]))
    if case == "ddpm":
        steps = int(f["diffusion_steps"])
        g, fx = _guidance(case, *shape, steps)
        tr = DDPMTrainer(sampler_namespace(cfg, ddim=False, diffusion_steps=steps), model)
        x, trace = tr.diffusion.p_sample_loop(model, shape, clip_denoised=False, cond_fn=g, noise_source=src, return_trace=True,
                                              model_kwargs=_kwargs(cfg, make_inputs(cfg, B, seed=int(f["input_seed"])), {}))
    else:
        g, fx = _guidance(case, *shape, 25)
        tr = DDPMTrainer(sampler_namespace(cfg), model)
        if case == "harmonize":
            _, inp, gt, mask = _masked(cfg, f)
            kw = _kwargs(cfg, inp, {"gt": gt, "outpainting_mask": mask})
        else:
            kw = _kwargs(cfg, make_inputs(cfg, B, seed=int(f["input_seed"])), {})
        x, trace = tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False, cond_fn=g, noise_source=src, return_trace=True,
                                                          eta=float(f["eta"]) if case == "eta" else 0.0, model_kwargs=kw)
    _RUNS[case] = (x.cpu(), trace, src.count, f, fx, base)
    return _RUNS[case]


@pytest.mark.parametrize("case", list(CASES))
def test_guided_loop_matches_reference(case):
    """plain: ddim25, all three terms.  harmonize: a masked window on the (3, 2) RePaint schedule, attraction.  eta: ddim25 at eta = 0.5,
    attraction + velocity under a per-level scale ramp.  ddpm: BEAT, the ancestral loop on a 50-step schedule, all three terms."""
    x, trace, draws, f, fx, base = _run_case(case)
    assert draws == int(f["draws"])
    if case == "harmonize":            # the fixture records denoise steps only; the trace also holds the undo steps
        from diffsheg_amd.diffusion import get_schedule_jump_cjm_ddim
        times = get_schedule_jump_cjm_ddim(25, 3, 2)
        trace = trace[[i for i, (a, b) in enumerate(zip(times[:-1], times[1:])) if b < a]]
    _check_trace(trace, f)
    ref = torch.from_numpy(f["final"])
    e, moved = rel_err(x, ref), rel_err(ref, base)
    print(f"[guided {case}] rel err {e:.3e}; the reference's guided sample differs from its unguided one by {moved:.3f} of the range")
    assert e < REL_TOL
    assert moved > 50 * REL_TOL, "the guidance of this fixture does not move the sample: the comparison shows nothing"


@pytest.mark.parametrize("case", list(CASES))
def test_attraction_brings_the_sample_nearer_its_targets(case):
    """The summed squared distance to Y over the keyed elements (W > 0) is strictly smaller with the guidance than in the reference's
    unguided sample of the same inputs and noise (it holds for the reference's own guided samples of all four fixtures, checked on the
    CPU when they were made) — strict reduction only, no ratio."""
    x, _, _, f, fx, base = _run_case(case)
    keyed = fx["weight"] > 0
    d_g = float(((x - fx["target"])[keyed].double() ** 2).sum())
    d_u = float(((base - fx["target"])[keyed].double() ** 2).sum())
    print(f"[behaviour {case}] distance to the targets: guided {d_g:.4g}, unguided {d_u:.4g}")
    assert d_g < d_u


# ---- 2. op level -------------------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _guide_c(dev, lens, scale, space):
    """(GuideC, objects to keep alive)"""
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    lh = None if lens is None else (C.c_int32 * len(lens))(*lens)
    g = _lib.GuideC(_p(dev.get("Y")), _p(dev.get("W")), _p(dev.get("lv")), _p(dev.get("la")), _p(ld), lh, scale, _lib.GUIDE_SPACES[space])
    return g, (ld, lh)


def _op_inputs(T, Cc, seed=0):
    B = 3
    gen = np.random.default_rng(1000 * T + Cc + seed)
    a = {"x": gen.standard_normal((B, T, Cc)) * 3, "eps": gen.standard_normal((B, T, Cc)), "n1": gen.standard_normal((B, T, Cc)),
         "hist": gen.standard_normal((B, T, Cc)), "Y": gen.standard_normal((B, T, Cc)), "W": gen.random((B, T, Cc)) * 0.5,
         "lv": gen.random(Cc) * 0.2, "la": gen.random(Cc) * 0.05}
    return {k: v.astype(np.float32).astype(np.float64) for k, v in a.items()}           # (fp32-representable: the kernel sees these very values)


def _scalars(k, eta=0.0):
    t = {n: diffusion_table(1000, 25, n) for n in ("alphas_cumprod", "alphas_cumprod_prev", "sqrt_recip_alphas_cumprod",
                                                   "sqrt_recipm1_alphas_cumprod")}
    ab, abp = np.float32(t["alphas_cumprod"][k]), np.float32(t["alphas_cumprod_prev"][k])
    sigma = np.float32(eta) * np.sqrt((1 - abp) / (1 - ab)) * np.sqrt(1 - ab / abp)
    A, Bc, G = solver_coeffs(1000, sorted(range(0, 1000, 40)), k)
    sc = {"c1": t["sqrt_recip_alphas_cumprod"][k], "c2": t["sqrt_recipm1_alphas_cumprod"][k], "sqrt_ab_prev": np.sqrt(abp),
          "coef_eps": np.sqrt(1 - abp - sigma * sigma), "sigma": sigma, "sqrt_1m_ab": np.sqrt(np.float32(1) - ab), "A": A, "Bc": Bc, "G": G}
    return {n: float(np.float32(v)) for n, v in sc.items()}


TERMS = {"all": ("Y", "W", "lv", "la"), "no_w": ("lv", "la"), "no_vel": ("Y", "W", "la"), "no_acc": ("Y", "W", "lv"), "w_no_y": ("W",)}


def _variants(T, Cc):
    split = get_config("show" if Cc == 232 else "beat").split_pos
    for terms in TERMS:
        for lens in (None, [T, 1, max(1, T - 2)]):
            for cols in ((0, 0), (0, split), (split, Cc)):
                yield terms, lens, cols


@pytest.mark.parametrize("Cc", [192, 232])
@pytest.mark.parametrize("T", [1, 2, 3, 5, 34])
def test_op_guidance_grad(T, Cc):
    a = _op_inputs(T, Cc)
    B, worst = 3, 0.0
    zd = torch.from_numpy(a["x"]).float().to(DEV)
    for terms, lens, cols in _variants(T, Cc):
        use = {k: a[k] for k in TERMS[terms]}
        dev = {k: torch.from_numpy(v).float().to(DEV) for k, v in use.items()}
        ref, e32 = R.yardstick(lambda: R.grad(a["x"], use.get("Y"), use.get("W"), use.get("lv"), use.get("la"), lens, 1.3),
                               lambda: R.grad(R.to_f32(a["x"]), *(R.to_f32(use.get(k)) for k in ("Y", "W", "lv", "la")), lens, 1.3))
        sent = torch.full((B, T, Cc), 777.0, device=DEV)
        g, keep = _guide_c(dev, lens, 1.3, "x_t")
        _lib.check(_lib.lib().dsh_op_guidance_grad(None, _p(zd), _p(sent), B, T, Cc, cols[0], cols[1], C.byref(g)), "dsh_op_guidance_grad")
        got = sent.cpu().double().numpy()
        lo, hi = cols if cols[1] > cols[0] else (0, Cc)
        assert (got[..., :lo] == 777.0).all() and (got[..., hi:] == 777.0).all(), "columns outside the range were written"
        if lens is not None:
            for b, L in enumerate(lens):
                assert (got[b, L:, lo:hi] == 0).all(), "frames beyond the clip's length carry a gradient"
        err = float(np.abs(got[..., lo:hi] - ref[..., lo:hi]).max())
        assert err <= GATE * e32, (terms, lens, cols, err, e32)
        worst = max(worst, err / e32) if e32 > 0 else worst
    print(f"[guidance_grad T {T} C {Cc}] worst kernel error / fp32 torch error = {worst:.3f}")


@pytest.mark.parametrize("Cc", [192, 232])
@pytest.mark.parametrize("T", [1, 2, 3, 5, 34])
def test_op_guided_steps(T, Cc):
    """dsh_op_guided_ddim_step (first order with the eta term, and the dpm2m form) and dsh_op_guided_ddpm_step in both spaces; elements
    outside the column range and frames beyond a clip's length stay their input bit for bit, in x and in the x0 history."""
    a = _op_inputs(T, Cc, seed=1)
    B, worst = 3, 0.0
    sc = _scalars(14, eta=0.5)
    scp = dict(sc, coef1=0.31, coef2=0.68, sigma=0.11, post_var=float(np.float32(0.0123)))
    x32, eps_d, n1_d = (torch.from_numpy(a[k]).float().to(DEV) for k in ("x", "eps", "n1"))
    h32 = torch.from_numpy(a["hist"]).float().to(DEV)
    f32 = {k: R.to_f32(a[k]) for k in a}
    for terms, lens, cols in _variants(T, Cc):
        use = {k: a[k] for k in TERMS[terms]}
        dev = {k: torch.from_numpy(v).float().to(DEV) for k, v in use.items()}
        gd = lambda src: {"Y": src.get("Y") if "Y" in use else None, "W": src.get("W") if "W" in use else None,
                          "lv": src.get("lv") if "lv" in use else None, "la": src.get("la") if "la" in use else None, "scale": 0.8}
        for space in ("x_t", "x0"):
            clip = space == "x0"
            g, keep = _guide_c(dev, lens, 0.8, space)
            for form in ("ddim", "dpm2m", "ddpm"):
                if form == "ddpm":
                    fn = lambda s: (R.guided_ddpm(s["x"], s["eps"], s["n1"], gd(s), scp, space, clip, lens, cols), None)
                else:
                    fn = lambda s: R.guided_ddim(s["x"], s["eps"], gd(s), sc, space, clip, lens, cols, noise1=s["n1"], hist=s["hist"],
                                                 second=form == "dpm2m")
                ref_x, ref_h = fn(a)
                y32, yh32 = fn(f32)
                e32 = float(np.abs(y32.double().numpy() - ref_x).max())
                xd, hd = x32.clone(), h32.clone()
                if form == "ddpm":
                    _lib.check(_lib.lib().dsh_op_guided_ddpm_step(None, _p(xd), _p(eps_d), _p(n1_d), None, C.byref(g), B, T, Cc, scp["c1"], scp["c2"],
                                                                  scp["coef1"], scp["coef2"], scp["sigma"], scp["post_var"], int(clip), *cols),
                               "dsh_op_guided_ddpm_step")
                else:
                    second = form == "dpm2m"
                    _lib.check(_lib.lib().dsh_op_guided_ddim_step(
                        None, _p(xd), _p(eps_d), _p(hd), None, None, None, None if second else _p(n1_d), C.byref(g), B, T, Cc, sc["c1"], sc["c2"],
                        sc["sqrt_ab_prev"], 0.0, sc["coef_eps"], sc["sigma"], sc["sqrt_1m_ab"], sc["A"], sc["Bc"], sc["G"], int(second), 0, 0, 0,
                        int(clip), *cols), "dsh_op_guided_ddim_step")
                got = xd.cpu().double().numpy()
                # untouched: bit for bit the input
                lo, hi = cols if cols[1] > cols[0] else (0, Cc)
                out = np.ones((B, T, Cc), dtype=bool)
                out[..., lo:hi] = False
                for b, L in enumerate(lens or []):
                    out[b, L:] = True
                assert (got[out] == a["x"][out]).all(), (form, space, terms, lens, cols)
                err = float(np.abs(got - ref_x).max())
                assert err <= GATE * e32, (form, space, terms, lens, cols, err, e32)
                worst = max(worst, err / e32) if e32 > 0 else worst
                if form != "ddpm":
                    goth = hd.cpu().double().numpy()
                    assert (goth[out] == a["hist"][out]).all(), (form, space, terms, lens, cols)
                    eh32 = float(np.abs(yh32.double().numpy() - ref_h).max())
                    assert float(np.abs(goth - ref_h).max()) <= GATE * eh32, (form, space, terms, lens, cols)
    print(f"[guided steps T {T} C {Cc}] worst kernel error / fp32 torch error = {worst:.3f}")


def test_op_entries_refuse_bad_arguments():
    lib = _lib.lib()
    z = torch.zeros(2, 6, 8, device=DEV)
    g, keep = _guide_c({"W": z}, None, 1.0, "x_t")
    assert lib.dsh_op_guidance_grad(None, _p(z), _p(z), 2, 6, 8, 0, 0, C.byref(g)) < 0                  # g aliases z
    out = torch.zeros_like(z)
    assert lib.dsh_op_guidance_grad(None, _p(z), _p(out), 2, 6, 8, 2, 9, C.byref(g)) < 0                # column range
    assert lib.dsh_op_guidance_grad(None, _p(z), _p(out), 2, 6, 8, 0, 0, None) < 0
    bad, keep2 = _guide_c({"W": z}, [6, 7], 1.0, "x_t")
    assert lib.dsh_op_guidance_grad(None, _p(z), _p(out), 2, 6, 8, 0, 0, C.byref(bad)) < 0 and b"clip length" in lib.dsh_last_error()
    half = _lib.GuideC(None, None, None, None, None, (C.c_int32 * 2)(6, 6), 1.0, 0)
    assert lib.dsh_op_guidance_grad(None, _p(z), _p(out), 2, 6, 8, 0, 0, C.byref(half)) < 0             # host lengths without the device copy
    g2, keep3 = _guide_c({"W": z}, None, 1.0, "x_t")
    g2.space = 5
    assert lib.dsh_op_guided_ddpm_step(None, _p(out), _p(z), _p(z), None, C.byref(g2), 2, 6, 8, 1, 1, 1, 1, 0, 0, 0, 0, 0) < 0
    assert b"space" in lib.dsh_last_error()
    assert lib.dsh_op_guided_ddim_step(None, _p(out), _p(z), None, None, None, None, None, C.byref(g), 2, 6, 8, 1, 1, 1, 0, 1, 0, 1, 1, 1, 1, 1,
                                       0, 0, 0, 0, 0, 0) < 0                                            # second order without the history
    assert float(out.abs().max()) == 0


# ---- 3. invariances ----------------------------------------------------------------------------------------------------------------
def test_guided_step_of_a_clip_does_not_depend_on_its_batch_or_the_column_range():
    """The step kernels themselves, bit for bit: clip 1 of a batch of 3 against the same clip alone, and a step on all columns against
    the two steps on the gesture and the expression columns."""
    T, Cc = 34, 232
    a = _op_inputs(T, Cc, seed=2)
    sc = _scalars(9)
    split = get_config("show").split_pos
    dev = {k: torch.from_numpy(a[k]).float().to(DEV) for k in a}
    for space in ("x_t", "x0"):
        for lens in (None, [T, 20, 7]):
            def run(rows, col_sets):
                x = dev["x"][rows].clone().contiguous()
                part = {k: dev[k][rows].contiguous() for k in ("Y", "W")}
                part.update(lv=dev["lv"], la=dev["la"])
                g, keep = _guide_c(part, None if lens is None else lens[rows], 1.0, space)
                for lo, hi in col_sets:
                    _lib.check(_lib.lib().dsh_op_guided_ddim_step(
                        None, _p(x), _p(dev["eps"][rows].contiguous()), None, None, None, None, None, C.byref(g), x.shape[0], T, Cc, sc["c1"], sc["c2"],
                        sc["sqrt_ab_prev"], 0.0, sc["coef_eps"], 0.0, sc["sqrt_1m_ab"], 0.0, 0.0, 0.0, 0, 0, 0, 0, 0, lo, hi))
                return x
            full = run(slice(0, 3), [(0, 0)])
            assert torch.equal(run(slice(1, 2), [(0, 0)])[0], full[1]), (space, lens)
            assert torch.equal(run(slice(0, 3), [(split, Cc), (0, split)]), full), (space, lens)


def _loop_setup(B, ds="show", precision="fp32", seed=61):
    cfg = get_config(ds)
    model = gpu_model(ds, precision)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    inp = make_inputs(cfg, B, seed=seed)
    shape = (B, cfg.n_poses, cfg.net_dim_pose)
    return cfg, model, tr, inp, shape


def test_pipelined_encoder_chains_are_bit_identical_when_guided(monkeypatch):
    """The two encoders' chains on two streams (DSH_PIPE, the switch of test_pipelined_encoder_chains_are_bit_identical) against the
    single chain, guided in both spaces, a plain and an out-painting window, and the DDPM loop: every term is local to its column."""
    _pipelined_chains_when_guided(3, "fp32", monkeypatch)


def test_pipelined_encoder_chains_are_bit_identical_when_guided_on_the_split_loop(monkeypatch):
    """precision "bf16x3", SHOW B = 6 (528 rows, above the 512-row limit of the split-bf16 loop): the pipelined twin instance reads the packed
    weights from the second stream."""
    _pipelined_chains_when_guided(6, "bf16x3", monkeypatch)


def _eager_run_is_on_the_split_loop(run, want, monkeypatch):
    """(graph replays pass no host-side counter: one eager loop, which must give the same bits, is the run that is counted)"""
    monkeypatch.setenv("DSH_NO_GRAPH", "1")
    _lib.launch_counts(reset=True)
    got = run()
    torch.cuda.synchronize()
    counts = _lib.launch_counts()
    monkeypatch.delenv("DSH_NO_GRAPH")
    assert torch.equal(got, want)
    assert_split_ran(counts, "guided loop")


def _pipelined_chains_when_guided(B, precision, monkeypatch):
    cfg, model, tr, inp, shape = _loop_setup(B, precision=precision)
    gt, mask = torch.zeros(shape), torch.zeros(shape, dtype=torch.bool)
    gt[:, :cfg.overlap_len] = torch.randn(B, cfg.overlap_len, shape[2], generator=torch.Generator().manual_seed(5))
    mask[:, :cfg.overlap_len] = True
    for space in ("x_t", "x0"):
        g, _ = _guidance("plain", *shape, 25, space)
        for y in ({}, {"gt": gt, "outpainting_mask": mask}):
            outs = []
            for pipe in ("1", "0", "1"):
                monkeypatch.setenv("DSH_PIPE", pipe)
                outs.append(tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=_kwargs(cfg, inp, y), seed=17,
                                                                   cond_fn=g).clone())
                assert _sample_flags()[1] == int(pipe), pipe
            assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), (space, bool(y))
            if precision == "bf16x3" and not y:
                _eager_run_is_on_the_split_loop(lambda: tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False, seed=17, cond_fn=g,
                                                                                              model_kwargs=_kwargs(cfg, inp, y)), outs[0], monkeypatch)
    trp = DDPMTrainer(sampler_namespace(cfg, ddim=False, diffusion_steps=50), model)
    g, _ = _guidance("ddpm", *shape, 50, "x0")
    outs = []
    for pipe in ("1", "0"):
        monkeypatch.setenv("DSH_PIPE", pipe)
        outs.append(trp.diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs=_kwargs(cfg, inp, {}), seed=23, cond_fn=g).clone())
    monkeypatch.delenv("DSH_PIPE")
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def _own_terms_only(tr, model, shape, kw, Y, W, vel, acc, probes, **loop_kw):
    """Bit for bit, at a fixed batch composition (the same evaluation kernels in every run): changing the target / weight of ONE row
    changes that row's sample and no other row's — every chain of the loop reads exactly its own rows of the guidance tensors."""
    B = shape[0]
    run = lambda y, w: tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False, seed=31, row_keys=list(range(B)), model_kwargs=kw,
                                                              cond_fn=MotionGuidance(y, w, vel, acc, space="x0"), **loop_kw).clone()
    base = run(Y, W)
    assert torch.isfinite(base).all() and torch.equal(run(Y, W), base)
    others = torch.ones(B, dtype=torch.bool)
    for b in probes:
        y2, w2 = Y.clone(), W.clone()
        y2[b] += 0.5
        w2[b] = w2[b] * 1.5 + 0.05        # (every element of the row: a short clip may hold none of the keyed frames)
        got = run(y2, w2)
        others[:] = True
        others[b] = False
        assert torch.equal(got[others], base[others]), f"row {b}'s terms reached another row"
        assert not torch.equal(got[b], base[b]), f"row {b} did not read its own terms"
    return base


UNGUIDED_ALONE = 1e-5      # a clip of a batched loop against the clip sampled alone, unguided: the bar of test_batch_rows_are_independent


def _alone_bound(W, vel, acc):
    """The bar for a GUIDED clip of a batched loop against the clip sampled alone, from the unguided one by reasoning, not by measuring.
    Evaluations of different batch sizes take different kernels, so the two loops see eps that differ in their last bits.  To first order
    (x0 space, no clip) the guided step is the unguided step composed with (I - gamma_k K): with x0 = c1 x - c2 eps the kernel computes
    x0' = x0 + c2 sqrt(1 - ab) g = (I - gamma_k K) x0, gamma_k = c2_k sqrt(1 - ab_k) s_k, where g = -s_k K z and K is the energy's
    (positive semi-definite) Hessian; both the eps and the x sensitivity of x_prev carry that factor (the x one with a smaller gamma).
    ||K|| <= kappa = max W + 4 max vel + 16 max acc (the norms of the identity, the first- and the second-difference Gram stencils).  So
    a difference that the unguided loop carries at UNGUIDED_ALONE may be carried larger by at most ||I - gamma_k K|| <= 1 + gamma_k kappa
    in a step; the bar takes that factor at the level where it is largest (the top one: gamma = c2 sqrt(1 - ab) ~ 1 / sqrt(ab))."""
    ab = diffusion_table(1000, 25, "alphas_cumprod")
    c2 = diffusion_table(1000, 25, "sqrt_recipm1_alphas_cumprod")
    gamma = float(np.max(c2 * np.sqrt(1.0 - ab)))
    kappa = float(W.max()) + 4 * float(vel.max()) + 16 * float(acc.max())
    return UNGUIDED_ALONE * (1.0 + gamma * kappa), gamma, kappa


@pytest.mark.parametrize("ragged", [False, True])
def test_sub_batch_streams_equal_the_rows_alone_and_read_their_own_guidance(ragged, monkeypatch):
    """SHOW fp32, B = 50 (two sub-batch streams, as test_sub_batch_streams_share_the_noise_scratch_by_offset), one Philox stream per row,
    full and ragged lengths: every chain is handed its element offset of target / weight and its clips' lengths.  Rows at the batch ends
    and on either side of the split (a) read exactly their own rows of the guidance tensors, bit for bit, and (b) equal the row sampled
    alone with its own terms within _alone_bound() of the range."""
    monkeypatch.setenv("DSH_PIPE", "0")
    B = 50
    cfg, model, tr, inp, shape = _loop_setup(B, seed=53)
    f = R.fixture_guidance("plain", 2, shape[1], shape[2], 25)
    rep = lambda v: v[:1].repeat(B, 1, 1) * torch.linspace(0.5, 1.5, B).view(B, 1, 1)          # every row its own targets and weights
    Y, W, vel, acc = rep(f["target"]).to(DEV), rep(f["weight"]).to(DEV), f["vel"].to(DEV), f["acc"].to(DEV)
    lens = [(shape[1], 40, 17, 60)[b % 4] for b in range(B)] if ragged else None
    kw = _kwargs(cfg, inp, {})
    if ragged:
        kw["length"] = torch.tensor(lens)
    probes = (0, 24, 25, 49)
    full = _own_terms_only(tr, model, shape, kw, Y, W, vel, acc, probes)
    assert _sample_flags()[2] == 2
    bound, gamma, kappa = _alone_bound(W, vel, acc)
    for b in probes:
        kw1 = _kwargs(cfg, {k: v[b:b + 1] for k, v in inp.items()}, {})
        if ragged:
            kw1["length"] = torch.tensor(lens[b:b + 1])
            assert lens[b] == shape[1] or float(full[b, lens[b]:].abs().max()) == 0
        solo = tr.diffusion_ddim_val.ddim_sample_loop(model, (1,) + shape[1:], clip_denoised=False, seed=31, row_keys=[b], model_kwargs=kw1,
                                                      cond_fn=MotionGuidance(Y[b:b + 1], W[b:b + 1], vel, acc, space="x0"))
        e = rel_err(solo[0], full[b])
        print(f"[guided, two sub-batch streams, ragged {ragged}] row {b} vs the row sampled alone: rel err {e:.3e} (bar {bound:.3e}: gamma {gamma:.1f}, kappa {kappa:.3f})")
        assert e < bound, b
    monkeypatch.delenv("DSH_PIPE")


def test_a_guided_clip_alone_equals_the_clip_in_a_batch_of_three():
    """B = 3, full and ragged lengths.  Bit for bit where it can be decided: the guided step kernel of a clip alone equals the clip's in a
    batch of 3 (test_guided_step_of_a_clip_does_not_depend_on_its_batch_or_the_column_range), and in the loop a row reads its own terms
    and lengths only (here).  The LOOP of a clip alone against the clip in a batch of 3 is not bit-identical in this project, guided or
    not: evaluations of different batch sizes take different kernels.  It is held to the unguided bar where unguided, and to
    _alone_bound() where guided (measured on MI355X: unguided 8.2e-07 / 7.6e-07, guided 3.0e-05 / 2.2e-05 of the range, full / ragged)."""
    B = 3
    cfg, model, tr, inp, shape = _loop_setup(B, seed=12)
    f = R.fixture_guidance("plain", *shape, 25)
    Y, W, vel, acc = (f[k].to(DEV) for k in ("target", "weight", "vel", "acc"))
    bound, gamma, kappa = _alone_bound(W, vel, acc)
    for lens in (None, [shape[1], 40, 17]):
        kw = _kwargs(cfg, inp, {})
        if lens is not None:
            kw["length"] = torch.tensor(lens)
        full = _own_terms_only(tr, model, shape, kw, Y, W, vel, acc, (0, 1, 2))
        if lens is not None:
            assert float(full[1, lens[1]:].abs().max()) == 0 and float(full[2, lens[2]:].abs().max()) == 0
        kw1 = _kwargs(cfg, {k: v[1:2] for k, v in inp.items()}, {})
        if lens is not None:
            kw1["length"] = torch.tensor(lens[1:2])
        for guided in (False, True):
            g = MotionGuidance(Y[1:2], W[1:2], vel, acc, space="x0") if guided else None
            gf = MotionGuidance(Y, W, vel, acc, space="x0") if guided else None
            solo = tr.diffusion_ddim_val.ddim_sample_loop(model, (1,) + shape[1:], clip_denoised=False, seed=31, row_keys=[1], cond_fn=g, model_kwargs=kw1)
            whole = tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False, seed=31, row_keys=[0, 1, 2], cond_fn=gf, model_kwargs=kw)
            e, bar = rel_err(solo[0], whole[1]), (bound if guided else UNGUIDED_ALONE)
            print(f"[clip alone vs in a batch of 3, lengths {lens}, guided {guided}] rel err {e:.3e} (bar {bar:.3e}), "
                  f"bit-identical {torch.equal(solo[0], whole[1])}")
            assert e < bar, (lens, guided)


def test_zero_guidance_is_the_unguided_sample_bit_for_bit():
    """level_scale all zeros, and W = 0 with no vel / acc, give exactly the unguided sample; so does cond_fn=None, which launches what
    the parent commit launches (the guided kernels are siblings: no argument of the existing launches changed)."""
    _zero_guidance(2, "fp32")


def test_zero_guidance_is_the_unguided_sample_bit_for_bit_on_the_split_loop(monkeypatch):
    """precision "bf16x3", SHOW B = 6 (528 rows): above the 512-row limit of the split-bf16 loop."""
    _zero_guidance(6, "bf16x3", monkeypatch)


def _zero_guidance(B, precision, monkeypatch=None):
    cfg, model, tr, inp, shape = _loop_setup(B, precision=precision, seed=7)
    kw = _kwargs(cfg, inp, {})
    f = R.fixture_guidance("plain", *shape, 25)
    run = lambda g, **k: tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False, seed=9, model_kwargs=kw, cond_fn=g, **k).clone()
    base = run(None)
    assert torch.isfinite(base).all()
    if precision == "bf16x3":
        _eager_run_is_on_the_split_loop(lambda: run(None), base, monkeypatch)
    for space in ("x_t", "x0"):
        zero_scale = MotionGuidance(f["target"].to(DEV), f["weight"].to(DEV), f["vel"].to(DEV), f["acc"].to(DEV), space=space, level_scale=[0.0] * 25)
        assert torch.equal(run(zero_scale), base), space
        zero_w = MotionGuidance(f["target"].to(DEV), torch.zeros(shape, device=DEV), space=space)
        assert torch.equal(run(zero_w), base), space
        assert not torch.equal(run(MotionGuidance(f["target"].to(DEV), f["weight"].to(DEV), space=space)), base), space
    lg = tr.diffusion_ddim_val
    base2 = lg.ddim_sample_loop(model, shape, clip_denoised=False, seed=9, model_kwargs=kw, solver="dpm2m").clone()
    zero_w = MotionGuidance(f["target"].to(DEV), torch.zeros(shape, device=DEV), space="x0")
    assert torch.equal(lg.ddim_sample_loop(model, shape, clip_denoised=False, seed=9, model_kwargs=kw, solver="dpm2m", cond_fn=zero_w), base2)


def test_refusals_on_a_context():
    B = 2
    cfg, model, tr, inp, shape = _loop_setup(B, seed=7)
    kw = _kwargs(cfg, inp, {})
    lg = tr.diffusion_ddim_val
    lg.ddim_sample_loop(model, shape, model_kwargs=kw, seed=1)      # (conditions the context for this shape: the refusals below change nothing)
    with pytest.raises(NotImplementedError):                      # any other callable, and denoised_fn, stay refused
        lg.ddim_sample_loop(model, shape, model_kwargs=kw, cond_fn=lambda x, t, **k: x)
    with pytest.raises(NotImplementedError):
        lg.ddim_sample_loop(model, shape, model_kwargs=kw, denoised_fn=lambda x: x)
    with pytest.raises(ValueError, match="sample shape"):
        lg.ddim_sample_loop(model, shape, model_kwargs=kw, cond_fn=MotionGuidance(torch.zeros(B, shape[1] - 1, shape[2], device=DEV)))
    with pytest.raises(ValueError, match="sample shape"):
        lg.ddim_sample_loop(model, shape, model_kwargs=kw, cond_fn=MotionGuidance(vel=torch.zeros(shape[2] - 1, device=DEV)))
    with pytest.raises(_lib.DshError, match="one entry per level"):
        lg.ddim_sample_loop(model, shape, model_kwargs=kw, cond_fn=MotionGuidance(vel=torch.zeros(shape[2], device=DEV), level_scale=[1.0] * 24))
    # the library's own shape refusal (a caller of the C interface): before anything changes in x
    x = torch.full(shape, 5.0, device=DEV)
    y = torch.zeros(shape, device=DEV)
    o = lg._opts(0, False, 1, 3)
    for fields, frag in ((dict(guide_target=y.data_ptr(), guide_batch=B + 1, guide_frames=shape[1], guide_channels=shape[2]), b"target / weight"),
                         (dict(guide_weight=y.data_ptr(), guide_batch=B, guide_frames=shape[1] + 1, guide_channels=shape[2]), b"target / weight"),
                         (dict(guide_vel=y.data_ptr(), guide_channels=shape[2] - 1), b"vel / acc"),
                         (dict(guide_acc=y.data_ptr(), guide_batch=B, guide_frames=shape[1]), b"vel / acc")):
        spec = _lib.run_spec(init=1, x=x.data_ptr(), guidance=1, **fields)
        cur = model._enter()
        try:
            rc = _lib.lib().dsh_sample_run(model._h, C.byref(o), C.byref(spec))
        finally:
            model._exit(cur)
        assert rc == -1 and frag in _lib.lib().dsh_last_error(), fields
    torch.cuda.synchronize()
    assert float((x - 5.0).abs().max()) == 0


# ---- 4. x0 space and the dpm2m solver, end to end ------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["ddim", "dpm2m"])
def test_x0_space_loop_against_a_float64_replay(solver):
    """SHOW, B = 2, 10 log-SNR steps, space="x0" with clip_denoised, all three terms, both solvers.  The loop is traced; for every step
    the device's own eps is the model handle's evaluation of the traced x at the step's timestep (the loop's evaluation, bit for bit:
    cache modes and graphs do not change an evaluation's bits), and the update is replayed on the host from the traced x in float64
    and in fp32 torch.  The device's next x has to sit within 4 x the fp32 run's error of the float64 one, step by step."""
    cfg = get_config("show")
    model = gpu_model("show", "fp32")
    kept = logsnr_timesteps(1000, 10)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    tr.set_sampling(10, "logsnr", solver)
    lg = tr.diffusion_ddim_val
    B = 2
    shape = (B, cfg.n_poses, cfg.net_dim_pose)
    inp = make_inputs(cfg, B, seed=3)
    kw = _kwargs(cfg, inp, {})
    g, fx = _guidance("plain", *shape, 10, "x0")
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(4))
    x, trace = lg.ddim_sample_loop(model, shape, noise=x_T, clip_denoised=True, model_kwargs=kw, seed=1, cond_fn=g, return_trace=True, solver=solver)
    assert torch.isfinite(x).all() and trace.shape[0] == 10
    tab = {n: diffusion_table_subset(1000, kept, n) for n in ("alphas_cumprod", "alphas_cumprod_prev", "sqrt_recip_alphas_cumprod",
                                                               "sqrt_recipm1_alphas_cumprod")}
    guide64 = {"Y": fx["target"].double().numpy(), "W": fx["weight"].double().numpy(), "lv": fx["vel"].double().numpy(),
               "la": fx["acc"].double().numpy(), "scale": 1.0}
    guide32 = {k: (R.to_f32(v) if k != "scale" else v) for k, v in guide64.items()}
    states = [x_T.to(DEV)] + [trace[i] for i in range(10)]
    hist64 = hist32 = None
    worst = 0.0
    for i, k in enumerate(range(9, -1, -1)):
        xi = states[i]
        ab, abp = np.float32(tab["alphas_cumprod"][k]), np.float32(tab["alphas_cumprod_prev"][k])
        c1, c2 = float(np.float32(tab["sqrt_recip_alphas_cumprod"][k])), float(np.float32(tab["sqrt_recipm1_alphas_cumprod"][k]))
        shape_e = (B, shape[1], cfg.expression_dim)
        eps = model(xi, torch.full((B,), kept[k], dtype=torch.long, device=DEV), sqrt_alphas=[torch.full(shape_e, c1), torch.full(shape_e, c2)],
                    audio_emb=inp["audio_emb"].cuda(), length=torch.full((B,), shape[1]), person_id=inp["person_id"].cuda(),
                    add_cond={"pretrain_aud_feat": inp["pretrain_aud_feat"].cuda()}, pe_type="pe_sinu", y={})
        A, Bc, G = solver_coeffs(1000, kept, k)
        sc = {"c1": c1, "c2": c2, "sqrt_ab_prev": float(np.sqrt(abp)), "coef_eps": float(np.sqrt(np.float32(1) - abp)), "sigma": 0.0,
              "sqrt_1m_ab": float(np.sqrt(np.float32(1) - ab)), "A": float(np.float32(A)), "Bc": float(np.float32(Bc)), "G": float(np.float32(G))}
        second = solver == "dpm2m" and i > 0 and k != 0
        x64, e64 = xi.cpu().double().numpy(), eps.cpu().double().numpy()
        if hist64 is None:
            hist64, hist32 = np.zeros_like(x64), torch.zeros(shape)
        ref, h64 = R.guided_ddim(x64, e64, guide64, sc, "x0", True, hist=hist64, second=second)
        y32, h32 = R.guided_ddim(xi.cpu(), eps.cpu(), guide32, sc, "x0", True, hist=hist32, second=second)
        # (the history of the next step is the device's: both replays restart from the traced state, so they carry their own x0)
        hist64, hist32 = h64, h32
        e32 = float(np.abs(y32.double().numpy() - ref).max())
        err = float(np.abs(states[i + 1].cpu().double().numpy() - ref).max())
        worst = max(worst, err / e32)
        print(f"[x0 {solver} step {i} level {k}] device error {err:.3e}, fp32 torch error {e32:.3e}")
        assert err <= GATE * e32, (i, k, err, e32)
    print(f"[x0 {solver}] worst device error / fp32 torch error = {worst:.3f}")


# ---- the RePaint select behind the guided update, op level ---------------------------------------------------------------------------
@pytest.mark.parametrize("T,L", [(5, 2), (34, 4)])
def test_op_guided_steps_with_the_repaint_select(T, L):
    """dsh_op_guided_ddim_step with a mask: the noised gt, the head cross-fade and the mirrored tail cross-fade act on the GUIDED update,
    in both spaces, first order and dpm2m, full and ragged lengths, all columns and the expression columns — against the float64
    restatement (tests/motion_guidance_ref.py: repaint()), same gate as the unmasked steps."""
    Cc, B = 232, 3
    a = _op_inputs(T, Cc, seed=3)
    gen = np.random.default_rng(T)
    a["gt"] = gen.standard_normal((B, T, Cc)).astype(np.float32).astype(np.float64)
    mask = np.zeros((B, T, Cc), dtype=bool)
    mask[:, :L] = True
    mask[:, T - L:] = True
    mask[:, :, ::7] = True                                # and some pinned columns
    sc = dict(_scalars(2), sqrt_1m_ab_prev=0.15)          # (a late level: the fades are on below 0.2)
    dev = {k: torch.from_numpy(v).float().to(DEV) for k, v in a.items()}
    mask_d = torch.from_numpy(mask).to(torch.uint8).to(DEV)
    f32 = {k: R.to_f32(v) for k, v in a.items()}
    split = get_config("show").split_pos
    worst = 0.0
    for space in ("x_t", "x0"):
        for second in (False, True):
            for lens in (None, [T, 1, max(1, T - 2)]):
                for cols in ((0, 0), (split, Cc)):
                    for tail_blend in (0, 1):
                        gd = lambda s: {"Y": s["Y"], "W": s["W"], "lv": s["lv"], "la": s["la"], "scale": 0.8}
                        rp = lambda s, m: {"mask": m, "gt": s["gt"], "noise2": s["n1"], "L": L, "blend": 1, "tail_blend": tail_blend}
                        fn = lambda s, m: R.guided_ddim(s["x"], s["eps"], gd(s), sc, space, space == "x0", lens, cols, hist=s["hist"], second=second,
                                                        rp=rp(s, m))
                        ref_x, ref_h = fn(a, mask)
                        y32, h32 = fn(f32, torch.from_numpy(mask))
                        e32 = float(np.abs(y32.double().numpy() - ref_x).max())
                        eh32 = float(np.abs(h32.double().numpy() - ref_h).max())
                        g, keep = _guide_c(dev, lens, 0.8, space)
                        xd, hd = dev["x"].clone(), dev["hist"].clone()
                        _lib.check(_lib.lib().dsh_op_guided_ddim_step(
                            None, _p(xd), _p(dev["eps"]), _p(hd), _p(dev["gt"]), _p(mask_d), _p(dev["n1"]), None, C.byref(g), B, T, Cc, sc["c1"], sc["c2"],
                            sc["sqrt_ab_prev"], sc["sqrt_1m_ab_prev"], sc["coef_eps"], 0.0, sc["sqrt_1m_ab"], sc["A"], sc["Bc"], sc["G"], int(second), L, 1,
                            tail_blend, int(space == "x0"), *cols), "dsh_op_guided_ddim_step")
                        err = float(np.abs(xd.cpu().double().numpy() - ref_x).max())
                        assert err <= GATE * e32, (space, second, lens, cols, tail_blend, err, e32)
                        assert float(np.abs(hd.cpu().double().numpy() - ref_h).max()) <= GATE * eh32, (space, second, lens, cols)
                        worst = max(worst, err / e32)
    print(f"[guided steps with RePaint T {T}] worst kernel error / fp32 torch error = {worst:.3f}")


# ---- the trainer's entry points --------------------------------------------------------------------------------------------------------
def test_trainer_entries_pass_the_guidance_on():
    """generate_batch(guidance=, lengths=) is the loop call with cond_fn=; sample_arbitrary_len(guidance=) with stream-long target / weight
    is the chain of per-window generate_batch calls on the cut terms (and with vel / acc alone the same object for every window);
    sample_inbetween and sample_variations steer what they re-sample and leave pinned / kept elements as they are.  Bit for bit."""
    from diffsheg_amd.trainer import get_windows, window_seed
    cfg = get_config("show")
    model = gpu_model("show", "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B, T, Cc, L = 2, cfg.n_poses, cfg.net_dim_pose, cfg.overlap_len
    step = T - L
    N = T + step + 30                                     # three windows, the last one shorter
    inp = make_inputs(cfg, B, frames=N, seed=21)
    audio, hub, pid = inp["audio_emb"].cuda(), inp["pretrain_aud_feat"].cuda(), inp["person_id"].cuda()
    gen = torch.Generator().manual_seed(5)
    Y = torch.randn(B, N, Cc, generator=gen).to(DEV)
    W = (torch.rand(B, N, Cc, generator=gen) < 0.05).float().to(DEV) * 0.2
    vel, acc = torch.full((Cc,), 0.03, device=DEV), torch.full((Cc,), 0.01, device=DEV)
    for g in (MotionGuidance(Y, W, vel, acc), MotionGuidance(vel=vel, acc=acc, space="x_t")):
        got = tr.sample_arbitrary_len(audio, pid, {"pretrain_aud_feat": hub}, seed=9, guidance=g)
        plain = tr.sample_arbitrary_len(audio, pid, {"pretrain_aud_feat": hub}, seed=9)
        assert tuple(got.shape) == (B, N, Cc) and torch.isfinite(got).all() and not torch.equal(got, plain)
        outs, prev = [], None
        wins = list(zip(get_windows(audio, T, step), get_windows(hub, T, step), get_windows(Y, T, step), get_windows(W, T, step)))
        assert len(wins) == 3 and wins[-1][0].shape[1] < T
        for ii, (a, h, y, w) in enumerate(wins):
            n = a.shape[1]
            gt = torch.zeros(B, n, Cc, device=DEV)
            mask = torch.zeros(B, n, Cc, dtype=torch.bool, device=DEV)
            if ii > 0:
                mask[:, :L] = True
                gt[:, :L] = prev[:, -L:]
            gw = g if g.target is None else MotionGuidance(y.contiguous(), w.contiguous(), vel, acc)
            prev = tr.generate_batch(a, pid, Cc, {"pretrain_aud_feat": h}, {"gt": gt, "outpainting_mask": mask, "outpainting_mask_any": ii > 0},
                                     seed=window_seed(9, ii), guidance=gw)
            outs.append(prev if ii == len(wins) - 1 else prev[:, :step])
        assert torch.equal(torch.cat(outs, 1), got)
    with pytest.raises(ValueError, match="stream-long"):
        tr.sample_arbitrary_len(audio, pid, {"pretrain_aud_feat": hub}, seed=9, guidance=MotionGuidance(Y[:, :T].contiguous(), W[:, :T].contiguous()))
    # one window: generate_batch against the loop call, ragged lengths included
    a1, h1 = audio[:, :T].contiguous(), hub[:, :T].contiguous()
    g1 = MotionGuidance(Y[:, :T].contiguous(), W[:, :T].contiguous(), vel, acc)
    for lens in (None, [T, 33]):
        got = tr.generate_batch(a1, pid, Cc, {"pretrain_aud_feat": h1}, {}, seed=4, guidance=g1, lengths=lens, row_keys=[0, 1])
        kw = {"audio_emb": a1, "length": torch.tensor(lens or [T, T]), "person_id": pid, "add_cond": {"pretrain_aud_feat": h1}, "y": {}, "pe_type": "pe_sinu"}
        want = tr.diffusion_ddim_val.ddim_sample_loop(model, (B, T, Cc), clip_denoised=False, model_kwargs=kw, seed=4, cond_fn=g1, row_keys=[0, 1])
        assert torch.equal(got, want) and not torch.equal(got, tr.generate_batch(a1, pid, Cc, {"pretrain_aud_feat": h1}, {}, seed=4, lengths=lens, row_keys=[0, 1]))
        if lens:
            assert float(got[1, 33:].abs().max()) == 0
    # in-betweening: the pinned frames stay pinned, the frames in between move
    head, tail = torch.randn(B, L, Cc, generator=gen).to(DEV), torch.randn(B, L, Cc, generator=gen).to(DEV)
    ib = tr.sample_inbetween(a1, pid, {"pretrain_aud_feat": h1}, head, tail, seed=6, guidance=g1)
    ib0 = tr.sample_inbetween(a1, pid, {"pretrain_aud_feat": h1}, head, tail, seed=6)
    assert torch.isfinite(ib).all() and not torch.equal(ib[:, L:T - L], ib0[:, L:T - L])
    assert torch.equal(ib[:, 0], ib0[:, 0]) and torch.equal(ib[:, T - 1], ib0[:, T - 1])
    # variations with a keep mask: kept elements are the input bit for bit, the rest is steered
    motions = torch.randn(B, T, Cc, generator=gen).to(DEV)
    keep = torch.zeros(B, T, Cc, dtype=torch.bool, device=DEV)
    keep[:, :, :60] = True
    va = tr.sample_variations(motions, a1, pid, {"pretrain_aud_feat": h1}, level=10, keep=keep, seed=8, guidance=g1)
    va0 = tr.sample_variations(motions, a1, pid, {"pretrain_aud_feat": h1}, level=10, keep=keep, seed=8)
    assert torch.equal(va[keep], motions[keep]) and not torch.equal(va[~keep], va0[~keep]) and torch.isfinite(va).all()
