"""Editing an existing take on a real MI355X: the q_sample kernel bit for bit against torch and against the Philox entries, the DDIM
loop restarted from a level (exact split property in every loop regime, fused "x holds x0" mode), the reference's own per-step functions
(fixtures of tests/golden/make_golden_editing.py), kept elements of a masked variation, and the DDIM reverse ODE.

No test here gates on a round trip: the synthetic weights are not a trained denoiser."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsheg_amd import _lib, glue  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.model import UniDiffuser  # noqa: E402
from diffsheg_amd.synthetic import SeededNoise, make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from util import assert_split_ran, golden, gpu_model, rel_err, synthetic_sd  # noqa: E402

DEV = "cuda:0"
REL_TOL = 1e-3          # tests/test_gpu_sampler.py: the fp32 gate of every reference loop fixture, relative to the output range
ROW_TOL = 1e-5          # tests/test_gpu_sampler.py::test_batch_rows_are_independent / tests/test_gpu_seam.py: the same rows at another batch size (fp32)
RESP = 25
M64 = (1 << 64) - 1


def _p(t):
    return C.c_void_p(t.data_ptr())


# ---- 1 / 2. the q_sample kernel --------------------------------------------------------------------------------------------------
def _q_op(x0, a, s, noise=None, c_lo=0, c_hi=0, fixed_from=-1, seed=0, offset=0, keys=None, seeds=None, lens=None, draw=0, sentinel=-77.0):
    B, T, Cc = x0.shape
    out = torch.full((B, T, Cc), sentinel, device=DEV)
    xd, ad, sd_ = x0.to(DEV), a.to(DEV), s.to(DEV)
    nd = None if noise is None else noise.to(DEV)
    karr = None if keys is None else (C.c_uint64 * B)(*keys)
    larr = None if lens is None else (C.c_int32 * B)(*lens)
    sdev = None if seeds is None else torch.tensor([v - (1 << 64) if v >> 63 else v for v in seeds], dtype=torch.int64).to(DEV)
    _lib.check(_lib.lib().dsh_op_q_sample(None, _p(out), _p(xd), None if nd is None else _p(nd), _p(ad), _p(sd_), B, T, Cc, c_lo, c_hi,
                                          fixed_from, seed, offset, karr, None if sdev is None else _p(sdev), larr, draw), "dsh_op_q_sample")
    torch.cuda.synchronize()
    return out.cpu()


def _case(shape, seed):
    g = torch.Generator().manual_seed(seed)
    B = shape[0]
    x0, n = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    a, s = torch.rand(B, generator=g) + 0.1, torch.rand(B, generator=g) + 0.1          # one pair per row
    return x0, n, a, s


def _torch_q(x0, n, a, s):
    return a.view(-1, 1, 1) * x0 + s.view(-1, 1, 1) * n                                 # fp32 on the CPU: mul, mul, add, each rounded


@pytest.mark.parametrize("shape", [(3, 5, 192), (2, 3, 4)])
def test_q_sample_with_given_noise_is_bit_exact(shape):
    x0, n, a, s = _case(shape, 7)
    Cc = shape[2]
    ref = _torch_q(x0, n, a, s)
    assert torch.equal(_q_op(x0, a, s, n), ref)
    lo, hi = 1, Cc - 1                                                                  # a column window: the rest is not written
    got = _q_op(x0, a, s, n, c_lo=lo, c_hi=hi)
    assert torch.equal(got[..., lo:hi], ref[..., lo:hi]) and bool((got[..., :lo] == -77.0).all()) and bool((got[..., hi:] == -77.0).all())
    ff = Cc // 2                                                                        # fixed_from: those columns are x0
    got = _q_op(x0, a, s, n, fixed_from=ff)
    assert torch.equal(got[..., :ff], ref[..., :ff]) and torch.equal(got[..., ff:], x0[..., ff:])
    got = _q_op(x0, a, s, n, c_lo=lo, c_hi=hi, fixed_from=ff)
    assert torch.equal(got[..., lo:ff], ref[..., lo:ff]) and torch.equal(got[..., ff:hi], x0[..., ff:hi]) and bool((got[..., hi:] == -77.0).all())
    # in place (the sampler's use): out = x0
    xd, nd, ad, sd_ = x0.to(DEV), n.to(DEV), a.to(DEV), s.to(DEV)
    _lib.check(_lib.lib().dsh_op_q_sample(None, _p(xd), _p(xd), _p(nd), _p(ad), _p(sd_), *shape, 0, 0, -1, 0, 0, None, None, None, 0))
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), ref)
    # the same buffers one float off the 16-byte grid (the float4 path does not apply): same values, nothing written outside
    nel = x0.numel()
    bufs = [torch.full((nel + 2,), -77.0, device=DEV) for _ in range(3)]
    bufs[1][1:nel + 1], bufs[2][1:nel + 1] = x0.reshape(-1).to(DEV), n.reshape(-1).to(DEV)
    _lib.check(_lib.lib().dsh_op_q_sample(None, *(C.c_void_p(t.data_ptr() + 4) for t in bufs), _p(ad), _p(sd_), *shape, 0, 0, -1, 0, 0, None, None, None, 0))
    torch.cuda.synchronize()
    got = bufs[0].cpu()
    assert torch.equal(got[1:nel + 1].view(shape), ref) and got[0] == -77.0 and got[nel + 1] == -77.0
    # given noise and lengths: padded frames are 0
    if shape[1] == 5:
        got = _q_op(x0, a, s, n, lens=[5, 3, 1])
        for b, ln in enumerate([5, 3, 1]):
            assert torch.equal(got[b, :ln], ref[b, :ln]) and bool((got[b, ln:] == 0).all())


def _philox(n, seed, offset):
    out = torch.empty(n, device=DEV)
    _lib.check(_lib.lib().dsh_op_philox_randn(None, _p(out), n, seed, offset), "dsh_op_philox_randn")
    torch.cuda.synchronize()
    return out.cpu()


def _philox_rows(keys, n_row, seed, offset=0, lens=None, draw=0, channels=0, seeds=None):
    rows = len(keys)
    out = torch.empty(rows, n_row, device=DEV)
    karr = (C.c_uint64 * rows)(*keys)
    larr = (C.c_int32 * rows)(*lens) if lens is not None else None
    sdev = None if seeds is None else torch.tensor([v - (1 << 64) if v >> 63 else v for v in seeds], dtype=torch.int64).to(DEV)
    _lib.check(_lib.lib().dsh_op_philox_randn_rows_ragged_seeded(None, _p(out), rows, n_row, seed, offset, karr, larr, draw, channels,
                                                                 None if sdev is None else _p(sdev)), "dsh_op_philox_randn_rows_ragged_seeded")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("shape", [(3, 5, 192), (2, 3, 4), (1, 3, 3)])
def test_q_sample_philox_forms_match_the_philox_entries(shape):
    x0, _, a, s = _case(shape, 9)
    B, T, Cc = shape
    n_row = T * Cc
    seed = 0x1234567890ABCDEF
    for off in (0, 5, (1 << 32) - 1):                                                   # whole tensor (the last quad may be partial)
        z = _philox(B * n_row, seed, off).view(shape)
        assert torch.equal(_q_op(x0, a, s, seed=seed, offset=off), _torch_q(x0, z, a, s)), off
    if n_row % 4:
        return
    keys = [3, 0xFFFFFFFF00000001, 17][:B]
    seeds = [0x8000000000000001, 5, 6][:B]
    for off in (0, 9):                                                                  # one stream per row; per-row Philox keys
        z = _philox_rows(keys, n_row, seed, off).view(shape)
        assert torch.equal(_q_op(x0, a, s, seed=seed, offset=off, keys=keys), _torch_q(x0, z, a, s))
        z = _philox_rows(keys, n_row, seed, off, seeds=seeds).view(shape)
        assert torch.equal(_q_op(x0, a, s, seed=seed, offset=off, keys=keys, seeds=seeds), _torch_q(x0, z, a, s))
    assert not torch.equal(_q_op(x0, a, s, seed=seed, keys=keys), _q_op(x0, a, s, seed=seed, keys=keys, seeds=seeds))
    if T != 5:
        return
    lens = [5, 3, 1]                                                                    # ragged rows: lengths * C / 4 quads per draw
    for draw in (0, 2):
        for sd_ in (None, seeds):
            z = _philox_rows(keys, n_row, seed, 0, lens=lens, draw=draw, channels=Cc, seeds=sd_).view(shape)
            ref = _torch_q(x0, z, a, s)
            got = _q_op(x0, a, s, seed=seed, keys=keys, seeds=sd_, lens=lens, draw=draw)
            for b, ln in enumerate(lens):
                assert torch.equal(got[b, :ln], ref[b, :ln]), (draw, b)
                assert bool((got[b, ln:] == 0).all()), (draw, b)
    # a window + fixed columns on the fused draw
    z = _philox_rows(keys, n_row, seed, 0).view(shape)
    ref = _torch_q(x0, z, a, s)
    got = _q_op(x0, a, s, seed=seed, keys=keys, c_lo=4, c_hi=100, fixed_from=90)
    assert torch.equal(got[..., 4:90], ref[..., 4:90]) and torch.equal(got[..., 90:100], x0[..., 90:100])
    assert bool((got[..., :4] == -77.0).all()) and bool((got[..., 100:] == -77.0).all())


def test_q_sample_op_refusals():
    x = torch.zeros(2, 3, 4, device=DEV)
    a = torch.ones(2, device=DEV)
    lib = _lib.lib()
    args = lambda **k: (None, _p(x), _p(x), k.get("n"), _p(a), _p(a), 2, 3, k.get("C", 4), 0, k.get("c_hi", 0), k.get("ff", -1), 1, 0,
                        k.get("keys"), None, k.get("lens"), 0)
    assert lib.dsh_op_q_sample(*args(c_hi=5)) < 0
    assert lib.dsh_op_q_sample(*args(ff=5)) < 0
    assert lib.dsh_op_q_sample(*args(lens=(C.c_int32 * 2)(1, 1))) < 0                   # ragged Philox needs the row keys
    assert lib.dsh_op_q_sample(*args(keys=(C.c_uint64 * 2)(1, 2), lens=(C.c_int32 * 2)(4, 1))) < 0
    assert lib.dsh_op_q_sample(*args(keys=(C.c_uint64 * 2)(1, 2), C=3)) < 0             # 9 values per row: no whole quads


def test_python_q_sample_matches_the_op_and_honours_fix_head_var():
    cfg = get_config("show")
    tr = DDPMTrainer(sampler_namespace(cfg), gpu_model("show", "fp32"))
    d = tr.diffusion_ddim_val
    g = torch.Generator().manual_seed(3)
    x0, n = torch.randn(3, 8, cfg.net_dim_pose, generator=g), torch.randn(3, 8, cfg.net_dim_pose, generator=g)
    t = torch.tensor([0, 9, 24])
    a, s = d.q_sample_coefficients(t, 3)
    assert torch.equal(d.q_sample(x0.to(DEV), t, n.to(DEV)).cpu(), _torch_q(x0, n, a, s))
    z = _philox(x0.numel(), 77, 0).view(x0.shape)
    assert torch.equal(d.q_sample(x0.to(DEV), t, seed=77).cpu(), _torch_q(x0, z, a, s))
    fhv = DDPMTrainer(sampler_namespace(cfg, fix_head_var=True), tr.encoder).diffusion_ddim_val
    got = fhv.q_sample(x0.to(DEV), 9, n.to(DEV)).cpu()
    assert torch.equal(got[..., 90:], x0[..., 90:]) and torch.equal(got[..., :90], _torch_q(x0, n, a[1:2].expand(3), s[1:2].expand(3))[..., :90])


def test_edit_region_builds_the_keep_mask():
    B, T, Cc = 3, 11, 7
    keep = glue.edit_region(B, T, Cc, frames=[(2, 5), (9, 11)], columns=[(0, 2), (6, 7)], device=DEV)
    ref = torch.ones(B, T, Cc, dtype=torch.bool)
    ref[:, 2:5] = False; ref[:, 9:11] = False; ref[:, :, 0:2] = False; ref[:, :, 6:7] = False
    assert keep.dtype == torch.bool and torch.equal(keep.cpu(), ref)
    keep = glue.edit_region(B, T, Cc, frames=torch.tensor([[0, 3], [4, 4], [10, 11]]), device=DEV)          # one range per row
    ref = torch.ones(B, T, Cc, dtype=torch.bool)
    ref[0, 0:3] = False; ref[2, 10:11] = False
    assert torch.equal(keep.cpu(), ref)
    assert bool(glue.edit_region(B, T, Cc, device=DEV).all())
    assert torch.equal(glue.edit_region(B, T, Cc, columns=[(3, 4)], device=DEV).cpu()[0, 0], torch.tensor([1, 1, 1, 0, 1, 1, 1], dtype=torch.bool))


# ---- loops -----------------------------------------------------------------------------------------------------------------------
def _kwargs(inp, y=None, **extra):
    B, T = inp["audio_emb"].shape[:2]
    kw = {"audio_emb": inp["audio_emb"], "length": torch.full((B,), T), "person_id": inp["person_id"],
          "add_cond": {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "y": {} if y is None else y, "pe_type": "pe_sinu"}
    kw.update(extra)
    return kw


def _flags():
    torch.cuda.synchronize()
    got = _lib.launch_counts()
    return got["sample_graph"], got["sample_pipe"], got["sample_streams"]


@functools.lru_cache(maxsize=None)
def _full_run(ds, precision, B, modality=False):
    """The plain ddim25 loop from noise with a trace (eta = 0: only draw 0 matters): (trainer, inputs, extra model kwargs, final, trace)."""
    cfg = get_config(ds)
    model = gpu_model(ds, precision)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    inp = make_inputs(cfg, B, seed=20 + B)
    extra = {}
    if modality:
        extra = {"modality": "gesture", "expression": torch.randn(B, cfg.n_poses, cfg.expression_dim, generator=torch.Generator().manual_seed(2))}
    x, trace = tr.diffusion_ddim_val.ddim_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False,
                                                      model_kwargs=_kwargs(inp, **extra), seed=5, return_trace=True)
    assert torch.isfinite(x).all() and trace.shape[0] == RESP
    return tr, inp, extra, x.clone(), trace.clone()


def _restart(tr, inp, extra, state, K, **kw):
    B, T, Cc = state.shape
    return tr.diffusion_ddim_val.ddim_sample_loop(tr.encoder, (B, T, Cc), noise=state, clip_denoised=False,
                                                  model_kwargs=_kwargs(inp, **extra), start_level=K, **kw)


# 3. the full schedule through the new argument: nothing moved
def test_full_schedule_through_start_level_is_the_existing_loop():
    cfg = get_config("show")
    model = gpu_model("show", "bf16")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B, T, Cc = 2, cfg.n_poses, cfg.net_dim_pose
    inp = make_inputs(cfg, B, seed=8)
    g = torch.Generator().manual_seed(1)
    xT = torch.randn(B, T, Cc, generator=g)
    loop = tr.diffusion_ddim_val.ddim_sample_loop
    base = loop(model, (B, T, Cc), noise=xT, clip_denoised=False, model_kwargs=_kwargs(inp), seed=3, eta=0.5).clone()
    got = loop(model, (B, T, Cc), noise=xT, clip_denoised=False, model_kwargs=_kwargs(inp), seed=3, eta=0.5, start_level=RESP)
    assert torch.isfinite(base).all() and torch.equal(base, got)
    # mask present: the built-in RePaint walk starts at t_T = 15 of ddim25, so 15 is its full schedule
    L = cfg.overlap_len
    gt = torch.zeros(B, T, Cc)
    gt[:, :L] = torch.randn(B, L, Cc, generator=g)
    mask = torch.zeros(B, T, Cc, dtype=torch.bool)
    mask[:, :L] = True
    y = {"gt": gt, "outpainting_mask": mask, "outpainting_mask_any": True}
    base = loop(model, (B, T, Cc), noise=xT, clip_denoised=False, model_kwargs=_kwargs(inp, y), seed=3).clone()
    got = loop(model, (B, T, Cc), noise=xT, clip_denoised=False, model_kwargs=_kwargs(inp, y), seed=3, start_level=15)
    assert torch.isfinite(base).all() and torch.equal(base, got)
    # ... and a mask-present run from the top level runs the longer walk (217 steps) and ends on the pinned frames as well
    top, trace = loop(model, (B, T, Cc), noise=xT, clip_denoised=False, model_kwargs=_kwargs(inp, y), seed=3, start_level=RESP, return_trace=True)
    assert trace.shape[0] == 217 and torch.isfinite(top).all() and torch.allclose(top[:, 0].cpu(), gt[:, 0], atol=1e-5)


# 4. split property: the loop restarted from its own traced state ends where the loop ended, bit for bit
# (precision "bf16x3": the smallest batches above the 512-row limit of the split-bf16 loop - below it the fp32 kernels run and the fp32 cases say it all)
RESTART_CASES = [(ds, precision, B) for ds in ("show", "beat") for precision in ("fp32", "bf16") for B in (1, 2)] + [("beat", "bf16x3", 16), ("show", "bf16x3", 6)]


@pytest.mark.parametrize("ds,precision,B", RESTART_CASES, ids=[f"{d}-{p}-{b}" for d, p, b in RESTART_CASES])
def test_restart_from_a_traced_state_is_bit_identical(ds, precision, B, monkeypatch):
    tr, inp, extra, final, trace = _full_run(ds, precision, B)
    for K in (1, 10, 24):
        state = trace[RESP - 1 - K]                      # after the step at level K: x at level K - 1
        # the default small-batch regime (graph replay + the two-encoder pipeline), the sequential loop, eager evaluations
        for env, want in (({}, (1, 1)), ({"DSH_PIPE": "0"}, (1, 0)), ({"DSH_NO_GRAPH": "1"}, (0, 1))):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            _lib.launch_counts(reset=True)
            got = _restart(tr, inp, extra, state, K, seed=99)
            flags = _flags()
            for k in env:
                monkeypatch.delenv(k)
            assert torch.equal(got, final), (K, env, float((got - final).abs().max()))
            if precision == "bf16x3" and "DSH_NO_GRAPH" in env:           # (eager evaluations: every launch passes the host-side counters)
                assert_split_ran(_lib.launch_counts(), (ds, B, K))
            if K == 10:
                assert flags == (want[0], want[1], 1), (env, flags)


def test_restart_on_forced_sub_batch_streams_is_bit_identical(monkeypatch):
    """Two sub-batch streams at B = 2: a context built under DSH_DUAL_MIN_ROWS / DSH_DUAL_ROWS splits 176 token rows, DSH_PIPE=0 keeps
    the loop from running them as one batch on the encoder pipeline."""
    ds, B = "show", 2
    cfg = get_config(ds)
    monkeypatch.setenv("DSH_DUAL_MIN_ROWS", "64")
    monkeypatch.setenv("DSH_DUAL_ROWS", "64")
    monkeypatch.setenv("DSH_PIPE", "0")
    model = UniDiffuser(cfg, synthetic_sd(ds), device=DEV, precision="bf16")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    inp = make_inputs(cfg, B, seed=22)
    shape = (B, cfg.n_poses, cfg.net_dim_pose)
    _lib.launch_counts(reset=True)
    final, trace = tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=_kwargs(inp), seed=5, return_trace=True)
    assert _flags()[2] == 2 and torch.isfinite(final).all()
    final = final.clone()
    for K in (1, 10, 24):
        _lib.launch_counts(reset=True)
        got = _restart(tr, inp, {}, trace[RESP - 1 - K], K, seed=99)
        assert _flags() == (0, 0, 2)
        assert torch.equal(got, final), K
    # the fused mode on the two streams: every chain noises its own rows
    x0 = torch.randn(*shape, generator=torch.Generator().manual_seed(4))
    _lib.launch_counts(reset=True)
    fused = tr.diffusion_ddim_val.ddim_sample_loop(model, shape, x_start=x0, clip_denoised=False, model_kwargs=_kwargs(inp), seed=31, start_level=10).clone()
    assert _flags()[2] == 2
    xk = tr.diffusion_ddim_val.q_sample(x0.to(DEV), 9, seed=31)
    two = _restart(tr, inp, {}, xk, 10, seed=31)
    assert torch.isfinite(fused).all() and torch.equal(fused, two)
    # the same two-stream split serves the reverse loop
    _lib.launch_counts(reset=True)
    inv = tr.diffusion_ddim_val.ddim_reverse_sample_loop(model, x0, 10, model_kwargs=_kwargs(inp)).clone()
    assert _flags()[2] == 2 and torch.isfinite(inv).all()
    again, trace = tr.diffusion_ddim_val.ddim_reverse_sample_loop(model, x0, 10, model_kwargs=_kwargs(inp), return_trace=True)
    assert torch.equal(inv, again) and torch.equal(trace[-1], again)


def test_restart_of_a_gesture_only_run_is_bit_identical():
    tr, inp, extra, final, trace = _full_run("show", "bf16", 2, True)
    G = tr.encoder.cfg.split_pos
    assert torch.equal(final[..., G:].cpu(), extra["expression"])
    for K in (1, 10, 24):
        got = _restart(tr, inp, extra, trace[RESP - 1 - K], K, seed=99)
        assert torch.equal(got, final), K


# 5. fused mode: x holds x0
@pytest.mark.parametrize("ds,precision", [("show", "fp32"), ("beat", "bf16")])
def test_fused_mode_is_q_sample_then_restart(ds, precision):
    cfg = get_config(ds)
    tr = DDPMTrainer(sampler_namespace(cfg), gpu_model(ds, precision))
    d = tr.diffusion_ddim_val
    B, K = 2, 10
    shape = (B, cfg.n_poses, cfg.net_dim_pose)
    inp = make_inputs(cfg, B, seed=12)
    x0 = torch.randn(*shape, generator=torch.Generator().manual_seed(6))
    for kw in ({}, {"row_keys": [41, 42]}, {"row_keys": [41, 42], "row_seeds": [7, M64]}):
        fused = d.ddim_sample_loop(tr.encoder, shape, x_start=x0, clip_denoised=False, model_kwargs=_kwargs(inp), seed=31, start_level=K, **kw).clone()
        xk = d.q_sample(x0.to(DEV), K - 1, seed=31, **kw)
        two = _restart(tr, inp, {}, xk, K, seed=31, **kw)
        assert torch.isfinite(fused).all() and torch.equal(fused, two), kw
        assert not torch.equal(fused.cpu(), x0)
    other = d.ddim_sample_loop(tr.encoder, shape, x_start=x0, clip_denoised=False, model_kwargs=_kwargs(inp), seed=32, start_level=K)
    assert not torch.equal(other, fused)
    # draw layout: draw 0 is the q_sample noise, the steps' draws follow from 1 (injected noise; eta != 0 so the values matter)
    src = SeededNoise(50)
    a = d.ddim_sample_loop(tr.encoder, shape, x_start=x0, clip_denoised=False, model_kwargs=_kwargs(inp), noise_source=src, start_level=K, eta=0.5).clone()
    assert src.count == K + 1
    src2 = SeededNoise(50)
    xk = d.q_sample(x0.to(DEV), K - 1, src2.randn(shape).to(DEV))

    class _From1:                                        # the restart takes no draw 0: hand it the stream from draw 1 on
        count = 0

        def randn(self, shp):
            return src2.randn(shp)
    b = _restart(tr, inp, {}, xk, K, noise_source=_From1(), eta=0.5)
    assert src2.count == K + 1 and torch.equal(a, b)


def test_fused_mode_rows_do_not_depend_on_their_batch():
    cfg = get_config("show")
    tr = DDPMTrainer(sampler_namespace(cfg), gpu_model("show", "fp32"))
    B, T, Cc = 3, cfg.n_poses, cfg.net_dim_pose
    inp = make_inputs(cfg, B, seed=14)
    cond = {"pretrain_aud_feat": inp["pretrain_aud_feat"]}
    x0 = torch.randn(B, T, Cc, generator=torch.Generator().manual_seed(8))
    keys, seeds = [11, 12, 13], [101, 102, 103]
    full = tr.sample_variations(x0, inp["audio_emb"], inp["person_id"], cond, level=10, seed=1, row_keys=keys, row_seeds=seeds).clone()
    worst = 0.0
    for b in range(B):
        solo = tr.sample_variations(x0[b:b + 1], inp["audio_emb"][b:b + 1], inp["person_id"][b:b + 1], {k: v[b:b + 1] for k, v in cond.items()},
                                    level=10, seed=2, row_keys=keys[b:b + 1], row_seeds=seeds[b:b + 1])
        worst = max(worst, rel_err(solo[0], full[b]))
    print(f"[variations, row keys + row seeds] worst rel err of a row vs the row alone: {worst:.3e}")
    assert worst < ROW_TOL


def test_fused_mode_on_a_ragged_batch_zeroes_the_padding():
    cfg = get_config("show")
    tr = DDPMTrainer(sampler_namespace(cfg), gpu_model("show", "bf16"))
    B, T, Cc = 2, cfg.n_poses, cfg.net_dim_pose
    inp = make_inputs(cfg, B, seed=15)
    x0 = torch.randn(B, T, Cc, generator=torch.Generator().manual_seed(9))
    lens = [T, T - 24]
    outs = [tr.sample_variations(x0, inp["audio_emb"], inp["person_id"], {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, strength=0.4, seed=3,
                                 row_keys=[5, 6], lengths=lens).clone() for _ in range(2)]
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    assert bool((outs[0][1, lens[1]:] == 0).all()) and bool((outs[0][1, :lens[1]] != 0).any())


# 6. the reference's own functions, level by level (fp32)
def _check_trace(trace, f, tag):
    corners = torch.from_numpy(f["step_corner"])
    got = trace[:, :, :3, :6].cpu()
    assert got.shape == corners.shape, (got.shape, corners.shape)
    worst = 0.0
    for i in range(corners.shape[0]):
        scale = float(f["step_stats"][i][2])            # max|x| of the reference at this step
        worst = max(worst, float((got[i] - corners[i]).abs().max()) / max(scale, 1.0))
    print(f"[{tag}] worst per-step corner err / range = {worst:.3e}")
    for i in range(corners.shape[0]):
        scale = float(f["step_stats"][i][2])
        assert float((got[i] - corners[i]).abs().max()) <= REL_TOL * max(scale, 1.0), f"step {i}"
        assert abs(float(trace[i].abs().mean()) - float(f["step_stats"][i][1])) <= 1e-4 * float(f["step_stats"][i][1]) + 1e-6
        assert abs(float(trace[i].abs().max()) - scale) <= REL_TOL * max(scale, 1.0)


def _fixture_setup(f, ds, **opt_over):
    cfg = get_config(ds)
    tr = DDPMTrainer(sampler_namespace(cfg, **opt_over), gpu_model(ds, "fp32"))
    B = int(f["batch"])
    inp = make_inputs(cfg, B, seed=int(f["input_seed"]))
    x0 = torch.randn(B, cfg.n_poses, cfg.net_dim_pose, generator=torch.Generator().manual_seed(int(f["x0_seed"])))
    return cfg, tr, B, inp, x0


@pytest.mark.parametrize("ds", ["show", "beat"])
def test_restart_matches_reference(ds):
    f = golden(f"edit_restart_{ds}.npz")
    cfg, tr, B, inp, x0 = _fixture_setup(f, ds)
    src = SeededNoise(int(f["noise_seed"]))
    x, trace = tr.diffusion_ddim_val.ddim_sample_loop(tr.encoder, tuple(x0.shape), x_start=x0, clip_denoised=False, model_kwargs=_kwargs(inp),
                                                      noise_source=src, start_level=int(f["level"]), return_trace=True)
    assert src.count == int(f["draws"]) == 11
    e = rel_err(x, torch.from_numpy(f["final"]))
    print(f"[edit restart {ds}] rel err {e:.3e}")
    _check_trace(trace, f, f"edit restart {ds}")
    assert e < REL_TOL


def test_keep_mask_restart_matches_reference():
    f = golden("edit_keep_show.npz")
    cfg, tr, B, inp, x0 = _fixture_setup(f, "show")
    keep = torch.zeros_like(x0, dtype=torch.bool)
    keep[:, :int(f["keep_frames"])] = True
    keep[:, :, :int(f["keep_cols"])] = True
    src = SeededNoise(int(f["noise_seed"]))
    y = {"gt": x0, "outpainting_mask": keep, "outpainting_mask_any": True}
    x, trace = tr.diffusion_ddim_val.ddim_sample_loop(tr.encoder, tuple(x0.shape), x_start=x0, clip_denoised=False, model_kwargs=_kwargs(inp, y),
                                                      noise_source=src, start_level=int(f["level"]), add_blend=False, return_trace=True)
    assert src.count == int(f["draws"]) == 129 and trace.shape[0] == int(f["steps"]) == 82
    e = rel_err(x, torch.from_numpy(f["final"]))
    print(f"[edit keep show] rel err {e:.3e}")
    _check_trace(trace, f, "edit keep show")
    assert e < REL_TOL
    assert torch.equal(x.cpu()[keep], x0[keep])


# 7. kept elements of a variation are the input
@pytest.mark.parametrize("ds,precision", [("show", "bf16"), ("beat", "fp32")])
def test_kept_elements_of_a_variation_are_the_input(ds, precision):
    cfg = get_config(ds)
    tr = DDPMTrainer(sampler_namespace(cfg), gpu_model(ds, precision))
    B, T, Cc = 2, cfg.n_poses, cfg.net_dim_pose
    inp = make_inputs(cfg, B, seed=16)
    cond = {"pretrain_aud_feat": inp["pretrain_aud_feat"]}
    x0 = torch.randn(B, T, Cc, generator=torch.Generator().manual_seed(10)).to(DEV)
    keep = glue.edit_region(B, T, Cc, frames=[(T // 3, T // 2)], columns=[(Cc - 9, Cc)], device=DEV)
    assert cfg.add_blend and 0 < int(keep.sum()) < keep.numel() and bool(keep[:, :cfg.overlap_len].any())      # the fade would touch kept frames
    outs = [tr.sample_variations(x0, inp["audio_emb"], inp["person_id"], cond, level=10, keep=keep, seed=s).clone() for s in (1, 1, 2)]
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    for o in outs:
        assert torch.equal(o[keep], x0[keep])
    edit = ~keep
    assert float((outs[0][edit] - x0[edit]).abs().mean()) > 1e-2
    assert float((outs[0][edit] - outs[2][edit]).abs().mean()) > 1e-3
    # a broadcast mask ([T, 1]: whole frames) and no mask at all
    frames_only = torch.zeros(T, 1, dtype=torch.bool)
    frames_only[:T // 2] = True
    o = tr.sample_variations(x0, inp["audio_emb"], inp["person_id"], cond, strength=0.2, keep=frames_only, seed=4)
    assert torch.equal(o[:, :T // 2], x0[:, :T // 2]) and not torch.equal(o[:, T // 2:], x0[:, T // 2:])
    free = tr.sample_variations(x0, inp["audio_emb"], inp["person_id"], cond, level=5, seed=4)
    assert torch.isfinite(free).all() and not torch.equal(free, x0)


# 8. the reverse ODE
# (no precision "bf16x3" case: the fixtures' batches are far below the 512-row limit of the split-bf16 loop, where that precision launches the
#  fp32 kernels; above the limit the reverse loop runs in the bit-equality test below, and against the oracle it is the forward loop's twin)
@pytest.mark.parametrize("ds", ["show", "beat"])
def test_reverse_loop_matches_reference(ds):
    f = golden(f"edit_invert_{ds}.npz")
    cfg, tr, B, inp, x0 = _fixture_setup(f, ds)
    d = tr.diffusion_ddim_val
    K = int(f["level"])
    x, trace = d.ddim_reverse_sample_loop(tr.encoder, x0, K, model_kwargs=_kwargs(inp), return_trace=True)
    e = rel_err(x, torch.from_numpy(f["final"]))
    print(f"[edit invert {ds}] rel err {e:.3e}")
    _check_trace(trace, f, f"edit invert {ds}")
    assert e < REL_TOL and trace.shape[0] == K
    # one step at a time through ddim_reverse_sample is the loop
    xs = x0
    for k in range(3):
        xs = d.ddim_reverse_sample(tr.encoder, xs, torch.full((B,), k), clip_denoised=False, model_kwargs=_kwargs(inp))["sample"]
        assert torch.equal(xs, trace[k]), k


@pytest.mark.parametrize("ds,precision,B", [("show", "bf16", 2), ("beat", "fp32", 1), ("show", "fp32", 3), ("beat", "bf16x3", 16)])
def test_pipelined_and_sequential_reverse_loops_are_bit_identical(ds, precision, B, monkeypatch):
    cfg = get_config(ds)
    tr = DDPMTrainer(sampler_namespace(cfg), gpu_model(ds, precision))
    inp = make_inputs(cfg, B, seed=18)
    x0 = torch.randn(B, cfg.n_poses, cfg.net_dim_pose, generator=torch.Generator().manual_seed(11))
    outs, flags = [], []
    for env in ({}, {"DSH_PIPE": "0"}, {"DSH_NO_GRAPH": "1"}, {}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _lib.launch_counts(reset=True)
        outs.append(tr.diffusion_ddim_val.ddim_reverse_sample_loop(tr.encoder, x0, 10, model_kwargs=_kwargs(inp)).clone())
        flags.append(_flags())
        if precision == "bf16x3" and "DSH_NO_GRAPH" in env:
            assert_split_ran(_lib.launch_counts(), (ds, B))
        for k in env:
            monkeypatch.delenv(k)
    assert flags == [(1, 1, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)], flags
    assert torch.isfinite(outs[0]).all() and not torch.equal(outs[0].cpu(), x0)
    for o in outs[1:]:
        assert torch.equal(outs[0], o)
    traced = tr.diffusion_ddim_val.ddim_reverse_sample_loop(tr.encoder, x0, 10, model_kwargs=_kwargs(inp), return_trace=True)[0]
    assert torch.equal(outs[0], traced)


def test_reverse_loop_ignores_row_keys_left_by_an_earlier_batch():
    """Row keys are sticky in the native context; the reverse loop draws nothing, so keys set for another batch size (a keyed variation
    at B = 3, ragged with keys at B = 3) must neither refuse nor change an inversion or a restyle at B = 2."""
    cfg = get_config("show")
    tr = DDPMTrainer(sampler_namespace(cfg), gpu_model("show", "bf16"))
    d = tr.diffusion_ddim_val
    T, Cc = cfg.n_poses, cfg.net_dim_pose
    inp3, inp2 = make_inputs(cfg, 3, seed=23), make_inputs(cfg, 2, seed=24)
    cond3, cond2 = {"pretrain_aud_feat": inp3["pretrain_aud_feat"]}, {"pretrain_aud_feat": inp2["pretrain_aud_feat"]}
    g = torch.Generator().manual_seed(13)
    x3, x2 = torch.randn(3, T, Cc, generator=g), torch.randn(2, T, Cc, generator=g)
    to = torch.roll(inp2["person_id"], 1, dims=-1)
    clean_inv = d.ddim_reverse_sample_loop(tr.encoder, x2, 10, model_kwargs=_kwargs(inp2)).clone()       # (follows an unkeyed state)
    clean_sty = tr.restyle(x2, inp2["audio_emb"], inp2["person_id"], to, cond2, level=10).clone()
    for kw in ({}, {"lengths": [T, T - 8, T - 16]}):
        tr.sample_variations(x3, inp3["audio_emb"], inp3["person_id"], cond3, level=5, seed=1, row_keys=[7, 8, 9], row_seeds=[1, 2, 3], **kw)
        inv = d.ddim_reverse_sample_loop(tr.encoder, x2, 10, model_kwargs=_kwargs(inp2))
        assert torch.equal(inv, clean_inv), kw
        tr.sample_variations(x3, inp3["audio_emb"], inp3["person_id"], cond3, level=5, seed=1, row_keys=[7, 8, 9], **kw)
        sty = tr.restyle(x2, inp2["audio_emb"], inp2["person_id"], to, cond2, level=10)
        assert torch.equal(sty, clean_sty), kw
    # keys set for the SAME batch size are not consulted either (a ragged reverse loop whose lengths * C are no multiples of 4 would be refused)
    tr.sample_variations(x2, inp2["audio_emb"], inp2["person_id"], cond2, level=5, seed=1, row_keys=[7, 8])
    assert torch.equal(d.ddim_reverse_sample_loop(tr.encoder, x2, 10, model_kwargs=_kwargs(inp2)), clean_inv)


def test_restyle_runs_is_deterministic_and_follows_the_target_speaker():
    cfg = get_config("show")
    tr = DDPMTrainer(sampler_namespace(cfg), gpu_model("show", "bf16"))
    B, T, Cc = 2, cfg.n_poses, cfg.net_dim_pose
    inp = make_inputs(cfg, B, seed=19)
    cond = {"pretrain_aud_feat": inp["pretrain_aud_feat"]}
    x0 = torch.randn(B, T, Cc, generator=torch.Generator().manual_seed(12))
    src = inp["person_id"]
    to_a, to_b = torch.roll(src, 1, dims=-1), torch.roll(src, 2, dims=-1)
    assert not torch.equal(to_a, src) and not torch.equal(to_a, to_b)
    a1 = tr.restyle(x0, inp["audio_emb"], src, to_a, cond, level=10).clone()
    a2 = tr.restyle(x0, inp["audio_emb"], src, to_a, cond, level=10).clone()
    b1 = tr.restyle(x0, inp["audio_emb"], src, to_b, cond, level=10)
    assert a1.shape == (B, T, Cc) and torch.isfinite(a1).all() and torch.isfinite(b1).all()
    assert torch.equal(a1, a2) and not torch.equal(a1, b1)
