"""Few-step sampling on a real MI355X: the DPM-Solver++(2M) step kernel one launch at a time against the fp32 restatement of
fewstep_ref.py (bit for bit), the native loops on a log-SNR subset against fixtures made with the reference's model and its own
SpacedDiffusion, the identities the solver must keep across the loop's regimes, the trainer's set_sampling, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fewstep_ref as F  # noqa: E402
from diffsheg_amd import _lib  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.diffusion import SpacedDiffusion, diffusion_table  # noqa: E402
from diffsheg_amd.synthetic import SeededNoise, make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace, window_seed  # noqa: E402
from util import assert_split_ran, golden, gpu_model, rel_err, synthetic_sd  # noqa: E402

DEV = "cuda:0"
REL_TOL = 1e-3                 # test_gpu_sampler.py: final and per-step corners against a reference fixture, relative to the range
SENTINEL, GUARD = 12345.0, 64


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _guarded(t):
    flat = torch.full((t.numel() + GUARD,), SENTINEL)
    flat[:t.numel()] = t.reshape(-1)
    return flat.to(DEV)


def _split(buf, shape):
    n = int(np.prod(shape))
    h = buf.cpu()
    return h[:n].reshape(shape), bool((h[n:] == SENTINEL).all())


def _spaced(cfg, kept, solver="ddim", **over):
    return SpacedDiffusion(use_timesteps=kept, solver=solver, rescale_timesteps=False, opt=sampler_namespace(cfg, **over),
                           betas=diffusion_table(1000, 0, "betas"))


def _kwargs(inp, y=None, lengths=None, **extra):
    B, T = inp["audio_emb"].shape[:2]
    kw = {"audio_emb": inp["audio_emb"], "length": torch.full((B,), T) if lengths is None else torch.tensor(lengths),
          "person_id": inp["person_id"], "add_cond": {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "y": y or {}, "pe_type": "pe_sinu"}
    kw.update(extra)
    return kw


def _outpaint(cfg, B, gt_seed=5):
    T, Cc, L = cfg.n_poses, cfg.net_dim_pose, cfg.overlap_len
    gt = torch.zeros(B, T, Cc)
    gt[:, :L] = torch.randn(B, L, Cc, generator=torch.Generator().manual_seed(gt_seed))
    mask = torch.zeros_like(gt, dtype=torch.bool)
    mask[:, :L] = True
    return {"gt": gt, "outpainting_mask": mask}


# ---- the op, one launch at a time --------------------------------------------------------------------------------------------------
def _op_inputs(shape, seed=7, L=4):
    g = torch.Generator().manual_seed(seed)
    B, T, Cc = shape
    t = {n: torch.randn(*shape, generator=g) for n in ("x", "eps", "hist", "gt", "nz2")}
    t["x"] *= 1.5
    mask = torch.zeros(shape, dtype=torch.bool)
    mask[:, :L] = True
    mask[:, T - L:] = True
    mask[:, T // 2, ::2] = True
    t["mask"] = mask
    return t


def _launch(t, sc, second, masked=False, L=0, blend=0, tail_blend=0, clip=0, win=(0, 0)):
    B, T, Cc = t["x"].shape
    c1, c2, sab, s1m, A, Bc, G = sc
    xd, hd = _guarded(t["x"]), _guarded(t["hist"])
    eps = t["eps"].to(DEV)
    gt, mk, nz = (t["gt"].to(DEV), t["mask"].to(torch.uint8).to(DEV), t["nz2"].to(DEV)) if masked else (None, None, None)
    _lib.check(_lib.lib().dsh_op_dpm2m_step(None, _p(xd), _p(eps), _p(hd), _p(gt), _p(mk), _p(nz), B, T, Cc, c1, c2, sab, s1m, A, Bc, G,
                                            int(second), L, blend, tail_blend, clip, win[0], win[1]), "dsh_op_dpm2m_step")
    torch.cuda.synchronize()
    (x, okx), (h, okh) = _split(xd, (B, T, Cc)), _split(hd, (B, T, Cc))
    assert okx and okh, "the step wrote behind n"
    return x, h


def _expect(t, sc, masked=False, L=0, blend=0, tail_blend=0, clip=0, win=(0, 0)):
    c1, c2, sab, s1m, A, Bc, G = sc
    kw = dict(sab=sab, s1m=s1m, mask=t["mask"], gt=t["gt"], nz2=t["nz2"], L=L, blend=blend, tail_blend=tail_blend) if masked else {}
    s, x0 = F.dpm2m_step(t["x"], t["eps"], t["hist"], c1, c2, A, Bc, G, clip=clip, **kw)
    return F.window(t["x"], s, *win), F.window(t["hist"], x0, *win)


TB10 = None


def _tb10():
    global TB10
    if TB10 is None:
        TB10 = F.kept_tables(1000, F.LOGSNR10)[0]
    return TB10


@pytest.mark.parametrize("shape", [(2, 11, 7), (1, 74913, 7)])
def test_dpm2m_step_is_bit_exact(shape):
    """n = 154: one partial block.  n = 524 391: past the 2048 x 256 grid, the stride loop wraps."""
    assert shape[1] * shape[0] * 7 in (154, 524391)
    t = _op_inputs(shape)
    sc = F.step_scalars(_tb10(), 5)
    for clip in (0, 1):
        x, h = _launch(t, sc, 1, clip=clip)
        wx, wh = _expect(t, sc, clip=clip)
        assert torch.equal(x, wx) and torch.equal(h, wh), (shape, clip, int((x != wx).sum()), int((h != wh).sum()))
        assert (not clip) or float(h.abs().max()) <= 1.0


def test_dpm2m_step_column_window_and_masked_forms():
    shape, L = (2, 11, 7), 4
    t = _op_inputs(shape, L=L)
    tb = _tb10()
    # a column window: the other columns of x and of the history keep their values
    sc = F.step_scalars(tb, 5)
    x, h = _launch(t, sc, 1, win=(3, 5))
    wx, wh = _expect(t, sc, win=(3, 5))
    assert torch.equal(x, wx) and torch.equal(h, wh)
    keep = [0, 1, 2, 5, 6]
    assert torch.equal(x[..., keep], t["x"][..., keep]) and torch.equal(h[..., keep], t["hist"][..., keep])
    assert not torch.equal(x[..., 3:5], t["x"][..., 3:5])
    # masked, at a level whose noise weight is below the fade threshold: plain select, head blend, head + mirrored tail blend
    sc = F.step_scalars(tb, 2)
    assert sc[3] < 0.2
    for blend, tail in ((0, 0), (1, 0), (1, 1)):
        for clip in (0, 1):
            for win in ((0, 0), (3, 5)):
                x, h = _launch(t, sc, 1, masked=True, L=L, blend=blend, tail_blend=tail, clip=clip, win=win)
                wx, wh = _expect(t, sc, masked=True, L=L, blend=blend, tail_blend=tail, clip=clip, win=win)
                assert torch.equal(x, wx) and torch.equal(h, wh), (blend, tail, clip, win, int((x != wx).sum()))
    a = _expect(t, sc, masked=True, L=L, blend=1, tail_blend=0)[0]
    b = _expect(t, sc, masked=True, L=L, blend=1, tail_blend=1)[0]
    assert not torch.equal(a[:, -L:], b[:, -L:]) and torch.equal(a[:, :-L], b[:, :-L])
    # refusals of the entry
    lib = _lib.lib()
    z = torch.zeros(1, 6, 8, device=DEV)
    m = torch.ones(1, 6, 8, dtype=torch.uint8, device=DEV)
    assert lib.dsh_op_dpm2m_step(None, _p(z), _p(z), None, None, None, None, 1, 6, 8, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0) < 0
    assert lib.dsh_op_dpm2m_step(None, _p(z), _p(z), _p(z), None, _p(m), None, 1, 6, 8, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0) < 0
    assert lib.dsh_op_dpm2m_step(None, _p(z), _p(z), _p(z), _p(z), _p(m), _p(z), 1, 6, 8, 1, 1, 1, 0, 1, 1, 1, 1, 4, 1, 1, 0, 0, 0) < 0
    assert b"tail_blend" in lib.dsh_last_error()
    assert lib.dsh_op_dpm2m_step(None, _p(z), _p(z), _p(z), None, None, None, 1, 6, 8, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0, 0, 0, 2, 9) < 0


def test_first_order_form_is_the_ddim_step():
    shape, L = (2, 11, 7), 4
    t = _op_inputs(shape, L=L)
    lib = _lib.lib()
    for k, masked in ((5, False), (2, True), (0, False)):
        c1, c2, sab, s1m, A, Bc, G = sc = F.step_scalars(_tb10(), k)
        for win in ((0, 0), (3, 5)):
            x, h = _launch(t, sc, 0, masked=masked, L=L, blend=int(masked), win=win)
            xd, x0d = _guarded(t["x"]), _guarded(t["hist"])
            gt, mk, nz = (t["gt"].to(DEV), t["mask"].to(torch.uint8).to(DEV), t["nz2"].to(DEV)) if masked else (None, None, None)
            _lib.check(lib.dsh_op_ddim_step_full(None, _p(xd), _p(t["eps"].to(DEV)), _p(x0d), _p(gt), _p(mk), _p(nz), None, None, None, 2, 11, 7,
                                                 c1, c2, sab, s1m, s1m, 0.0, L, int(masked), 0, 0, win[0], win[1]), "dsh_op_ddim_step_full")
            torch.cuda.synchronize()
            assert torch.equal(x, _split(xd, shape)[0]) and torch.equal(h, _split(x0d, shape)[0]), (k, masked, win)


def test_ten_step_op_loop_is_second_order():
    """logsnr10 on 154 values, eps of the analytic denoiser (data ~ N(0, s^2)) computed on the host in fp32 each step: the op loop equals the
    fp32 restatement bit for bit, and its error against the closed-form answer is >= 4 x smaller than the DDIM-op loop's."""
    shape, s = (2, 11, 7), 0.5
    tb, _ = F.kept_tables(1000, F.LOGSNR10)
    ac = tb["alphas_cumprod"]
    xT = torch.randn(*shape, generator=torch.Generator().manual_seed(3))
    exact = xT.double() * np.sqrt(s * s / (ac[9] * s * s + 1 - ac[9]))

    def eps_of(x, k):
        return x * torch.tensor(np.float32(np.sqrt(1 - ac[k]) / (ac[k] * s * s + 1 - ac[k])))

    errs = {}
    for solver in ("ddim", "dpm2m"):
        x, hist = xT.clone(), torch.zeros(shape)
        xr, hr = xT.clone(), None
        for k in range(9, -1, -1):
            second = solver == "dpm2m" and k != 0 and k != 9
            sc = F.step_scalars(tb, k)
            x, hist = _launch({"x": x, "eps": eps_of(x, k), "hist": hist}, sc, second)
            if second:
                xr, hr = F.dpm2m_step(xr, eps_of(xr, k), hr, sc[0], sc[1], sc[4], sc[5], sc[6])
            else:
                xr, hr = F.ddim_step_f32(xr, eps_of(xr, k), *sc[:4])
            assert torch.equal(x, xr) and torch.equal(hist, hr), (solver, k, int((x != xr).sum()), float((x - xr).abs().max()),
                                                                  int((hist != hr).sum()), float((hist - hr).abs().max()))
        errs[solver] = float(((x.double() - exact).abs() / xT.double().abs()).max())
    print(f"[op loop logsnr10, s = {s}] error per unit of x_T: ddim {errs['ddim']:.3e}, dpm2m {errs['dpm2m']:.3e}, ratio {errs['ddim'] / errs['dpm2m']:.2f}")
    assert errs["ddim"] / errs["dpm2m"] >= 4.0


# ---- the native loop against the fixtures ------------------------------------------------------------------------------------------
def _check_trace(trace, f, prefix):
    """test_gpu_sampler.py::_check_trace on the fixture's `prefix` records"""
    corners, stats = torch.from_numpy(f[prefix + "step_corner"]), f[prefix + "step_stats"]
    got = trace[:, :, :3, :6].cpu()
    assert got.shape == corners.shape, (got.shape, corners.shape)
    for i in range(corners.shape[0]):
        scale = float(stats[i][2])
        assert float((got[i] - corners[i]).abs().max()) <= REL_TOL * max(scale, 1.0), f"step {i}"
        assert abs(float(trace[i].abs().mean()) - float(stats[i][1])) <= 1e-4 * float(stats[i][1]) + 1e-6
        assert abs(float(trace[i].abs().max()) - scale) <= REL_TOL * max(scale, 1.0)


def _fixture_run(precision, which):
    cfg = get_config("beat")
    f = golden("fewstep_plain_beat.npz")
    model = gpu_model("beat", precision)
    B, shape = int(f["batch"]), (int(f["batch"]), cfg.n_poses, cfg.net_dim_pose)
    kept = [int(v) for v in f["kept"]]
    assert kept == F.LOGSNR8
    if which == "masked":
        inp = make_inputs(cfg, B, seed=int(f["masked_input_seed"]))
        y = _outpaint(cfg, B, gt_seed=int(f["masked_gt_seed"]))             # (the fixture's gt: one randn of [B, L, C] from that seed)
        src = SeededNoise(int(f["masked_noise_seed"]))
    else:
        inp, y, src = make_inputs(cfg, B, seed=int(f["input_seed"])), {}, SeededNoise(int(f["noise_seed"]))
    d = _spaced(cfg, kept, "ddim" if which == "ddim" else "dpm2m")
    x, trace = d.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=_kwargs(inp, y), noise_source=src, return_trace=True)
    return f, x, trace, src


@pytest.mark.parametrize("which", ["ddim", "dpm"])
def test_logsnr8_plain_loops_match_the_fixtures(which):
    """ddim: the reference's own ddim_sample_loop on the logsnr8 set.  dpm: the restated dpm2m loop driven by the reference's model."""
    f, x, trace, src = _fixture_run("fp32", which)
    assert src.count == int(f[which + "_draws"]) == 9
    _check_trace(trace, f, which + "_")
    e = rel_err(x, torch.from_numpy(f[which + "_final"]))
    print(f"[logsnr8 {which} beat fp32] rel err {e:.3e}")
    assert e < REL_TOL


def test_logsnr8_masked_window_matches_the_fixture():
    f, x, trace, src = _fixture_run("fp32", "masked")
    times = [int(v) for v in f["masked_times"]]
    assert int(f["masked_t_T"]) == times[0] + 1 and src.count == int(f["masked_draws"])
    den = [i for i, (a, b) in enumerate(zip(times[:-1], times[1:])) if b < a]
    assert trace.shape[0] == len(times) - 1
    _check_trace(trace[den], f, "masked_")
    e = rel_err(x, torch.from_numpy(f["masked_final"]))
    print(f"[logsnr8 dpm2m masked beat fp32] t_T {times[0] + 1}, {len(den)} evaluations, rel err {e:.3e}")
    assert e < REL_TOL


def test_bf16_logsnr8_dpm2m_error_beside_ddim25():
    """bf16 against the fp32 fixture, gated at 3 x the ddim25 bf16 figure of test_bf16_ddim25_end_to_end_error_vs_reference measured in
    this run (the margin that test keeps over its own measurement)."""
    cfg = get_config("show")
    f25 = golden("ddim25_plain_show.npz")
    model = gpu_model("show", "bf16")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B = int(f25["batch"])
    inp = make_inputs(cfg, B, seed=int(f25["input_seed"]))
    x25 = tr.diffusion_ddim_val.ddim_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False, model_kwargs=_kwargs(inp),
                                                 noise_source=SeededNoise(int(f25["noise_seed"])))
    e25 = rel_err(x25, torch.from_numpy(f25["final"]))
    f, x, _, _ = _fixture_run("bf16", "dpm")
    e8 = rel_err(x, torch.from_numpy(f["dpm_final"]))
    print(f"[bf16 end to end] logsnr8 dpm2m beat: max err / range = {e8:.3e};  ddim25 show (this run): {e25:.3e};  gate 3 x = {3 * e25:.3e}")
    assert e8 < 3 * e25


def test_logsnr8_dpm2m_on_the_split_loop_matches_the_replay():
    """precision "bf16x3", BEAT B = 16 (544 rows: the smallest batch on the split-bf16 loop; the fixtures' batch is below the limit and
    would run the fp32 kernels): the 8-evaluation DPM-Solver++(2M) loop against fewstep_ref.sample_loop driven by the CPU oracle on the same
    injected noise, under the fixtures' gate of 1e-3 of the range.  The fp32 path's distance on the same run is printed beside it."""
    from oracle import denoiser_ref, sampler_ref
    cfg, sd = get_config("beat"), synthetic_sd("beat")
    B = 16
    shape = (B, cfg.n_poses, cfg.net_dim_pose)
    inp = make_inputs(cfg, B, seed=77)
    d = _spaced(cfg, F.LOGSNR8, "dpm2m")

    def eps_fn(xc, t_orig, c1, c2):
        with torch.no_grad():
            return denoiser_ref.unidiffuser(sd, cfg, xc, torch.full((B,), t_orig), c1, c2, inp["audio_emb"], inp["person_id"], inp["pretrain_aud_feat"])
    ref = F.sample_loop(eps_fn, shape, None, sampler_ref.NoiseSource(seed=9), F.LOGSNR8, solver="dpm2m", overlap_len=cfg.overlap_len)
    errs = {}
    for precision in ("bf16x3", "fp32"):
        src = SeededNoise(9)
        _lib.launch_counts(reset=True)
        x = d.ddim_sample_loop(gpu_model("beat", precision), shape, clip_denoised=False, model_kwargs=_kwargs(inp), noise_source=src)
        torch.cuda.synchronize()
        c = _lib.launch_counts()
        assert src.count == 9 and torch.isfinite(x).all()
        if precision == "bf16x3":
            assert_split_ran(c, "logsnr8 dpm2m")
        else:
            assert c["gemm_f32_split"] == 0
        errs[precision] = rel_err(x, ref)
    print(f"[measure] logsnr8 dpm2m beat B={B} against the replay on the oracle: bf16x3 {errs['bf16x3']:.3e} of the range (fp32: {errs['fp32']:.3e})")
    assert errs["bf16x3"] < REL_TOL


# ---- identities, bit for bit -------------------------------------------------------------------------------------------------------
def _pair(ds, precision, B, kept, y=None, seed=5, trace=False, **kw):
    cfg = get_config(ds)
    model = gpu_model(ds, precision)
    inp = make_inputs(cfg, B, seed=40 + B)
    shape = (B, cfg.n_poses, cfg.net_dim_pose)
    out = []
    for solver in ("ddim", "dpm2m"):
        r = _spaced(cfg, kept, solver).ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=_kwargs(inp, y), seed=seed,
                                                        return_trace=trace, **kw)
        out.append(tuple(t.clone() for t in r) if trace else r.clone())
    return out


def test_up_to_two_steps_the_solvers_are_one_loop():
    for kept in ([600], [300, 900]):
        a, b = _pair("beat", "fp32", 2, kept)
        assert torch.isfinite(a).all() and torch.equal(a, b), kept
    cfg = get_config("beat")
    a, b = _pair("beat", "fp32", 2, [300, 900], y=_outpaint(cfg, 2))
    assert torch.equal(a, b)


def test_first_step_and_x_T_are_shared():
    (a, ta), (b, tb) = _pair("beat", "fp32", 2, F.LOGSNR8, trace=True)
    assert torch.equal(ta[0], tb[0])                       # same x_T, and the first step is first order under either solver
    assert not torch.equal(ta[1], tb[1]) and not torch.equal(a, b)
    # the last step is first order too: from the same state it gives the same bits (restart at level 0 from the dpm2m run's state)
    cfg = get_config("beat")
    model = gpu_model("beat", "fp32")
    inp = make_inputs(cfg, 2, seed=42)
    outs = [_spaced(cfg, F.LOGSNR8, s).ddim_sample_loop(model, tuple(b.shape), noise=tb[-2], start_level=1, clip_denoised=False,
                                                        model_kwargs=_kwargs(inp), seed=5).clone() for s in ("ddim", "dpm2m")]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], b)


@pytest.mark.parametrize("ds,precision,B", [("show", "bf16", 1), ("beat", "fp32", 3)])
def test_pipelined_chains_are_bit_identical(ds, precision, B, monkeypatch):
    cfg = get_config(ds)
    model = gpu_model(ds, precision)
    d = _spaced(cfg, F.LOGSNR10, "dpm2m")
    inp = make_inputs(cfg, B, seed=31 + B)
    shape = (B, cfg.n_poses, cfg.net_dim_pose)
    for name, y in (("plain", {}), ("outpaint", _outpaint(cfg, B))):
        outs, pipes = [], []
        for pipe in ("1", "0", "1"):
            monkeypatch.setenv("DSH_PIPE", pipe)
            outs.append(d.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=_kwargs(inp, y), seed=17).clone())
            torch.cuda.synchronize()
            pipes.append(_lib.launch_counts()["sample_pipe"])
        assert pipes == [1, 0, 1], (name, pipes)
        assert torch.isfinite(outs[0]).all(), name
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), (name, float((outs[0] - outs[1]).abs().max()))
    monkeypatch.delenv("DSH_PIPE")


def test_sub_batch_streams_equal_the_whole_batch(monkeypatch):
    """SHOW bf16, B = 200 (test_gpu_dispatch_sweep.py's mid-size batch): one batch on the encoder pipeline (default) against two sub-batch
    streams (DSH_PIPE=0); every clip runs the same kernels in both, and every stream addresses its own rows of the history."""
    _streams_against_the_whole_batch("bf16", 200, monkeypatch)


def test_sub_batch_streams_equal_the_whole_batch_on_the_split_loop(monkeypatch):
    """SHOW bf16x3, B = 47 (4 136 rows: the first batch fp32 storage splits over two streams, and above the graph range): the whole batch
    has every layer Linear on the 128 x 128 tile (8 272 rows with the null half), its two halves keep the N = 512 ones - the StylizationBlock
    Linears with the CFG-null row constant among them - on 64 x 64: the bits of the split loop do not depend on the tile."""
    _streams_against_the_whole_batch("bf16x3", 47, monkeypatch)


def _streams_against_the_whole_batch(precision, B, monkeypatch):
    cfg = get_config("show")
    model = gpu_model("show", precision)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    tr.set_sampling(10, "logsnr", "dpm2m")
    T, Cc = cfg.n_poses, cfg.net_dim_pose
    small = make_inputs(cfg, 64, frames=T, seed=23)
    rep = (B + 63) // 64
    audio = small["audio_emb"].repeat(rep, 1, 1)[:B].cuda().contiguous()
    hub = small["pretrain_aud_feat"].repeat(rep, 1, 1)[:B].cuda().contiguous()
    audio += 0.01 * torch.randn(audio.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    pid = torch.zeros(B, cfg.style_dim, device=DEV)
    pid[torch.arange(B), torch.arange(B) % cfg.style_dim] = 1.0
    outs, streams = {}, {}
    for env in ("1", "0"):
        monkeypatch.setenv("DSH_PIPE", env)
        _lib.launch_counts(reset=True)
        outs[env] = tr.generate_batch(audio.clone(), pid.clone(), Cc, {"pretrain_aud_feat": hub.clone()}, {}, seed=11,
                                      row_keys=list(range(300, 300 + B))).clone()
        torch.cuda.synchronize()
        streams[env] = _lib.launch_counts()["sample_streams"]
        if precision == "bf16x3":
            assert_split_ran(_lib.launch_counts(), env)
    monkeypatch.delenv("DSH_PIPE")
    assert streams == {"1": 1, "0": 2}, streams
    assert torch.isfinite(outs["1"]).all() and torch.equal(outs["1"], outs["0"]), float((outs["1"] - outs["0"]).abs().max())


def test_timestep_cache_on_and_off(monkeypatch):
    cfg = get_config("show")
    model = gpu_model("show", "fp32")
    d = _spaced(cfg, F.LOGSNR10, "dpm2m")
    B = 2
    kw = _kwargs(make_inputs(cfg, B, seed=21), _outpaint(cfg, B, 4))
    shape = (B, cfg.n_poses, cfg.net_dim_pose)
    a = d.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, seed=11).clone()
    monkeypatch.setenv("DSH_LEVEL_CACHE", "0")
    b = d.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, seed=11).clone()
    monkeypatch.delenv("DSH_LEVEL_CACHE")
    monkeypatch.setenv("DSH_LEVEL_PREFETCH", "0")
    c = d.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, seed=11).clone()
    monkeypatch.delenv("DSH_LEVEL_PREFETCH")
    assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c)


def test_ragged_row_is_the_clip_alone():
    """Lengths 88 and 31 in one batch: the short row equals the clip sampled alone at 31 frames from the same row key, bit for bit, and
    its padded frames are 0.  The DDIM solver's figure on the same inputs is printed beside it."""
    cfg = get_config("show")
    model = gpu_model("show", "fp32")
    B, T, Cc, lens, keys = 2, cfg.n_poses, cfg.net_dim_pose, [88, 31], [71, 72]
    assert T == 88
    inp = make_inputs(cfg, B, frames=T, seed=61)
    errs = {}
    for solver in ("ddim", "dpm2m"):
        d = _spaced(cfg, F.LOGSNR10, solver)
        full = d.ddim_sample_loop(model, (B, T, Cc), clip_denoised=False, model_kwargs=_kwargs(inp, lengths=lens), seed=9, row_keys=keys).clone()
        assert torch.isfinite(full).all() and float(full[1, 31:].abs().max()) == 0.0
        solo_in = {k: v[1:2, :31].contiguous() if v.dim() == 3 else v[1:2] for k, v in inp.items()}
        solo = d.ddim_sample_loop(model, (1, 31, Cc), clip_denoised=False, model_kwargs=_kwargs(solo_in), seed=9, row_keys=keys[1:])
        errs[solver] = (rel_err(full[1, :31], solo[0]), torch.equal(full[1, :31], solo[0]))
    print(f"[ragged 88 / 31, logsnr10] short row vs the clip alone: dpm2m rel err {errs['dpm2m'][0]:.3e} (bit-equal: {errs['dpm2m'][1]}), "
          f"ddim {errs['ddim'][0]:.3e} (bit-equal: {errs['ddim'][1]})")
    assert errs["dpm2m"][1]


def test_expression_modality_is_the_joint_run():
    cfg = get_config("show")
    model = gpu_model("show", "bf16")
    d = _spaced(cfg, F.LOGSNR10, "dpm2m")
    B, G = 2, cfg.net_dim_pose - cfg.expression_dim
    inp = make_inputs(cfg, B, seed=77)
    shape = (B, cfg.n_poses, cfg.net_dim_pose)
    joint = d.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=_kwargs(inp), seed=3).clone()
    part = d.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=_kwargs(inp, modality="expression"), seed=3).clone()
    assert torch.isfinite(joint).all() and torch.equal(part[..., G:], joint[..., G:]) and not part[..., :G].any()


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------
def test_set_sampling_chain_equals_the_windows_fed_by_hand():
    cfg = get_config("beat")
    model = gpu_model("beat", "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    tr.set_sampling(10, "logsnr", "dpm2m")
    assert tr.diffusion_ddim_val.timestep_map == F.LOGSNR10 and tr.diffusion_ddim_val.solver == "dpm2m"
    B, T, L, Cc = 2, cfg.n_poses, cfg.overlap_len, cfg.net_dim_pose
    step = T - L
    N = T + 2 * step
    inp = make_inputs(cfg, B, frames=N, seed=13)
    a, p, h = inp["audio_emb"].cuda(), inp["person_id"].cuda(), inp["pretrain_aud_feat"].cuda()
    chain = tr.sample_arbitrary_len(a, p, {"pretrain_aud_feat": h}, seed=7, row_keys=[3, 4]).clone()
    assert chain.shape == (B, N, Cc) and torch.isfinite(chain).all()
    d = _spaced(cfg, F.LOGSNR10, "dpm2m")
    prev, outs = None, []
    for i in range(3):
        sl = slice(i * step, i * step + T)
        y = {"gt": torch.zeros(B, T, Cc), "outpainting_mask": torch.zeros(B, T, Cc, dtype=torch.bool)}
        if i > 0:
            y["gt"][:, :L] = prev[:, -L:].cpu()
            y["outpainting_mask"][:, :L] = True
        w_in = {"audio_emb": a[:, sl], "person_id": p, "pretrain_aud_feat": h[:, sl]}
        prev = d.ddim_sample_loop(model, (B, T, Cc), clip_denoised=False, model_kwargs=_kwargs(w_in, y), seed=window_seed(7, i),
                                  row_keys=[3, 4]).clone()
        outs.append(prev if i == 2 else prev[:, :step])
    assert torch.equal(chain, torch.cat(outs, dim=1))


def test_set_sampling_defaults_and_variations():
    cfg = get_config("beat")
    model = gpu_model("beat", "fp32")
    B, Cc = 2, cfg.net_dim_pose
    inp = make_inputs(cfg, B, seed=15)
    a, p, cnd = inp["audio_emb"].cuda(), inp["person_id"].cuda(), {"pretrain_aud_feat": inp["pretrain_aud_feat"].cuda()}
    fresh = DDPMTrainer(sampler_namespace(cfg), model).generate_batch(a, p, Cc, cnd, {}, seed=3).clone()
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    tr.set_sampling(10, "logsnr", "dpm2m")
    few = tr.generate_batch(a, p, Cc, cnd, {}, seed=3).clone()
    assert torch.isfinite(few).all() and not torch.equal(few, fresh)
    # level= counts in the current step count; the first step of the restart is first order (K = 4: the state after it equals ddim's)
    motions = torch.randn(B, cfg.n_poses, Cc, generator=torch.Generator().manual_seed(8))
    with pytest.raises(ValueError):
        tr.sample_variations(motions, a, p, cnd, level=11, seed=2)
    var = tr.sample_variations(motions, a, p, cnd, level=4, seed=2)
    assert var.shape == motions.shape and torch.isfinite(var).all()
    traces = []
    for solver in ("ddim", "dpm2m"):
        _, t = _spaced(cfg, F.LOGSNR10, solver).ddim_sample_loop(model, tuple(motions.shape), x_start=motions, start_level=4, clip_denoised=False,
                                                                 model_kwargs=_kwargs(inp), seed=2, return_trace=True)
        traces.append(t.clone())
    assert traces[0].shape[0] == 4 and torch.equal(traces[0][0], traces[1][0]) and not torch.equal(traces[0][1], traces[1][1])
    assert torch.equal(traces[1][-1], var)
    # restyle runs on the subset (reverse ODE on its tables, first order) and the defaults give today's object back
    out = tr.restyle(motions, a, p, p.flip(0), cnd, level=3)
    assert torch.isfinite(out).all()
    # in-betweening (a mask pinned at both ends, the mirrored tail fade) and chains of different lengths run on the same object
    L, T = cfg.overlap_len, cfg.n_poses
    head, tail = motions[:, :L], motions[:, -L:]
    mid = tr.sample_inbetween(a, p, cnd, head, tail, seed=4)
    assert torch.isfinite(mid).all() and torch.allclose(mid[:, 0].cpu(), head[:, 0], atol=1e-5) and torch.allclose(mid[:, -1].cpu(), tail[:, -1], atol=1e-5)
    N = T + (T - L)
    long_in = make_inputs(cfg, B, frames=N, seed=16)
    la, lh = long_in["audio_emb"].cuda(), long_in["pretrain_aud_feat"].cuda()
    lens = [N, N - 7]
    outs = tr.sample_arbitrary_len(la, p, {"pretrain_aud_feat": lh}, seed=5, row_keys=[8, 9], lengths=lens)
    assert [tuple(o.shape) for o in outs] == [(n, Cc) for n in lens] and all(torch.isfinite(o).all() for o in outs)
    solo = tr.sample_arbitrary_len(la[:1], p[:1], {"pretrain_aud_feat": lh[:1]}, seed=5, row_keys=[8])
    assert rel_err(outs[0], solo[0]) < 1e-5                          # (test_gpu_ragged.py: a chain of a ragged fp32 batch vs the chain alone)
    tr.set_sampling()
    assert tr.diffusion_ddim_val._kept is None and tr.diffusion_ddim_val.num_timesteps == 25
    assert torch.equal(tr.generate_batch(a, p, Cc, cnd, {}, seed=3), fresh)
    opt = sampler_namespace(cfg)
    opt.sampling_steps, opt.sampling_spacing, opt.solver = 8, "logsnr", "dpm2m"
    assert DDPMTrainer(opt, model).diffusion_ddim_val.timestep_map == F.LOGSNR8


# ---- refusals: raised / returned before any state changes ------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was():
    cfg = get_config("beat")
    model = gpu_model("beat", "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B, T, Cc = 2, cfg.n_poses, cfg.net_dim_pose
    inp = make_inputs(cfg, B, seed=19)
    kw, shape = _kwargs(inp), (B, T, Cc)
    base = tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, seed=1).clone()

    def unchanged():
        assert torch.equal(tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, seed=1), base)

    d = _spaced(cfg, F.LOGSNR10)
    with pytest.raises(ValueError, match="eta"):
        d.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, seed=1, solver="dpm2m", eta=0.5)
    with pytest.raises(ValueError, match="solver"):
        d.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, seed=1, solver="heun")
    with pytest.raises(NotImplementedError, match="same_overlap_noisy"):
        _spaced(cfg, F.LOGSNR10, same_overlap_noisy=True).ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, seed=1, solver="dpm2m")
    with pytest.raises(TypeError):
        tr.diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, seed=1, solver="dpm2m")
    for bad in ("heun", 3):
        with pytest.raises(ValueError):
            tr.set_sampling(10, "logsnr", bad)
    for bad in ("cosine", [1, 2, 3], [5, 5, 9, 10, 11, 12, 13, 14, 15, 16]):
        with pytest.raises(ValueError):
            tr.set_sampling(10, bad)
    assert tr.diffusion_ddim_val.num_timesteps == 25
    unchanged()
    # the C surface: the context answers -1 and keeps sampling as before
    lib, h = _lib.lib(), model._h
    x = torch.zeros(shape, device=DEV)
    arr = (C.c_int32 * 10)(*F.LOGSNR10)
    for bad in ([5, 5, 9], [9, 5], [-1, 4]):
        assert lib.dsh_sample_set_timesteps(h, (C.c_int32 * len(bad))(*bad), len(bad)) < 0, bad
    assert lib.dsh_sample_set_solver(h, 2) < 0 and b"solver" in lib.dsh_last_error()
    unchanged()
    try:
        _lib.check(lib.dsh_sample_set_timesteps(h, arr, 10))
        o = tr.diffusion_ddim_val._opts(0, False, 1, 1)                  # respacing 25 against a list of 10
        assert lib.dsh_sample(h, C.byref(o), _p(x), 0, None, None, 0, None, 0, None) == -1 and b"respacing" in lib.dsh_last_error()
        o = tr.diffusion._opts(1, False, 1, 1)
        assert lib.dsh_sample(h, C.byref(o), _p(x), 0, None, None, 0, None, 0, None) == -1 and b"DDIM" in lib.dsh_last_error()
        big = (C.c_int32 * 10)(*(F.LOGSNR10[:-1] + [1000]))
        _lib.check(lib.dsh_sample_set_timesteps(h, big, 10))
        o = d._opts(0, False, 1, 1)
        assert lib.dsh_sample(h, C.byref(o), _p(x), 0, None, None, 0, None, 0, None) == -1 and b"outside" in lib.dsh_last_error()
        _lib.check(lib.dsh_sample_set_timesteps(h, arr, 0))
        _lib.check(lib.dsh_sample_set_solver(h, 1))
        o = tr.diffusion_ddim_val._opts(0, False, 1, 1, eta=0.5)
        assert lib.dsh_sample(h, C.byref(o), _p(x), 0, None, None, 0, None, 0, None) == -1 and b"eta" in lib.dsh_last_error()
        o = tr.diffusion_ddim_val._opts(0, False, 1, 1)
        o.same_overlap_noisy = 1
        assert lib.dsh_sample(h, C.byref(o), _p(x), 0, None, None, 0, None, 0, None) == -1 and b"same_overlap_noisy" in lib.dsh_last_error()
        o = tr.diffusion._opts(1, False, 1, 1)
        assert lib.dsh_sample(h, C.byref(o), _p(x), 0, None, None, 0, None, 0, None) == -1 and b"DDIM loops only" in lib.dsh_last_error()
    finally:
        lib.dsh_sample_set_timesteps(h, arr, 0)
        lib.dsh_sample_set_solver(h, 0)
    unchanged()
    # the reverse ODE ignores the solver
    x0 = torch.randn(shape, generator=torch.Generator().manual_seed(6))
    inv = d.ddim_reverse_sample_loop(model, x0, 4, model_kwargs=kw).clone()
    _lib.check(lib.dsh_sample_set_solver(h, 1))
    try:
        assert torch.equal(d.ddim_reverse_sample_loop(model, x0, 4, model_kwargs=kw), inv)
    finally:
        lib.dsh_sample_set_solver(h, 0)
    unchanged()
