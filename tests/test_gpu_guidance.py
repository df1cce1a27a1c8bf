"""Runtime and per-clip classifier-free guidance scale on a real MI355X (UniDiffuser.set_guidance_scale, opt.cond_scale /
cond_scale= of the sampling loops, dsh_set_guidance_scale).

  * parity with the imported reference at runtime scales (tests/golden/guidance_show.npz, ddim25_guidance_show.npz);
  * one context at a runtime scale == a context created at that scale, bit for bit (same kernels, same shapes);
  * per-clip scales: row b of a mixed batch == row b of the uniform run at s_b, bit for bit, in every regime the sampler picks;
  * the argument rules of the Python and C interfaces.

The models here are private to this module (the session-wide handles of tests/util.py keep their own sticky setting)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsheg_amd import _lib  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.model import MotionTransformer, UniDiffuser  # noqa: E402
from diffsheg_amd.synthetic import SeededNoise, make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from diffsheg_amd.weights import make_synthetic_state_dict  # noqa: E402
from oracle import denoiser_ref  # noqa: E402
from util import assert_split_ran, golden, max_abs, rel_err, synthetic_sd  # noqa: E402

FP32_ATOL = 1e-3                       # test_gpu_eval's golden tolerance
BF16_MAX, BF16_RMS = 6e-2, 1.5e-2      # test_gpu_eval's bf16 gates
REL_TOL = 1e-3                         # test_gpu_sampler's end-to-end gate
BF16_E2E_REL = 1.2e-2
MIXED = [1.15, 2.0, 0.0, 1.25]         # per-clip scales, none of them 1 (cycled over the batch)

_MODELS = {}


def _model(precision="fp32", cond_scale=1.25, ds="show", single=False):
    key = (ds, precision, cond_scale, single)
    if key not in _MODELS:
        cfg = get_config(ds, cond_scale=cond_scale, unidiffuser=not single)
        cls = MotionTransformer if single else UniDiffuser
        sd = make_synthetic_state_dict(cfg, 1234) if single else synthetic_sd(ds)
        _MODELS[key] = cls(cfg, sd, device="cuda:0", precision=precision)
    m = _MODELS[key]
    m.set_guidance_scale(None)
    return m


def _eval(model, inp, t=560, c1=4.9, c2=4.8):
    cfg = model.cfg
    B, T = inp["x_T"].shape[:2]
    shape_e = (B, T, cfg.expression_dim)
    if isinstance(model, MotionTransformer):
        return model(inp["x_T"].cuda(), torch.full((B,), t, dtype=torch.long).cuda(), inp["audio_emb"].cuda(), None,
                     inp["person_id"].cuda(), {"pretrain_aud_feat": inp["pretrain_aud_feat"].cuda()}, "pe_sinu", {})
    return model(inp["x_T"].cuda(), torch.full((B,), t, dtype=torch.long).cuda(),
                 sqrt_alphas=[torch.full(shape_e, float(c1)), torch.full(shape_e, float(c2))], audio_emb=inp["audio_emb"].cuda(),
                 length=None, person_id=inp["person_id"].cuda(), add_cond={"pretrain_aud_feat": inp["pretrain_aud_feat"].cuda()},
                 pe_type="pe_sinu", y={})


def _kwargs(inp, y=None):
    return {"audio_emb": inp["audio_emb"], "length": None, "person_id": inp["person_id"],
            "add_cond": {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "y": {} if y is None else y, "pe_type": "pe_sinu"}


def _ddim(model, inp, y=None, opt=None, **kw):
    cfg = model.cfg
    tr = DDPMTrainer(opt or sampler_namespace(cfg), model)
    B, T = inp["x_T"].shape[:2]
    kw.setdefault("seed", 4321)
    return tr.diffusion_ddim_val.ddim_sample_loop(model, (B, T, cfg.net_dim_pose), clip_denoised=False, model_kwargs=_kwargs(inp, y), **kw)


def _scales(B, scales=MIXED):
    return [scales[b % len(scales)] for b in range(B)]


# ---- 1. reference parity ------------------------------------------------------------------------------------------------
def test_runtime_scales_match_reference_fp32():
    f = golden("guidance_show.npz")
    cfg = get_config("show")
    model = _model("fp32", 1.25)
    inp = make_inputs(cfg, int(f["batch"]), seed=int(f["input_seed"]))
    for st, s in (("s100", 1.0), ("s115", 1.15), ("s200", 2.0)):
        model.set_guidance_scale(s)
        for tag in ("k0", "k14"):
            eps = _eval(model, inp, int(f[f"{tag}_t"]), float(f[f"{tag}_c1"]), float(f[f"{tag}_c2"]))
            ref = torch.from_numpy(np.concatenate([f[f"{tag}_{st}_eps_ges"], f[f"{tag}_{st}_eps_exp"]], axis=-1))
            e = max_abs(eps, ref)
            print(f"[guidance fp32 {st} {tag}] max|eps - ref| = {e:.3e}")
            assert e < FP32_ATOL, (st, tag, e)
            assert max_abs(eps[..., cfg.split_pos:], torch.from_numpy(f[f"{tag}_{st}_eps_exp"])) < FP32_ATOL
        if s == 1.0:
            # the values cannot show it: at 1 the null half is not evaluated at all (transformer.py:537)
            flops_runtime = model.eval_flops()
            baked = _model("fp32", 1.0)
            _eval(baked, inp, int(f["k14_t"]), float(f["k14_c1"]), float(f["k14_c2"]))
            assert flops_runtime == baked.eval_flops()
            model.set_guidance_scale(None)
            _eval(model, inp, int(f["k14_t"]), float(f["k14_c1"]), float(f["k14_c2"]))
            assert model.eval_flops() > 1.5 * flops_runtime
    model.set_guidance_scale(None)


def test_runtime_scale_bf16_close_to_reference():
    f = golden("guidance_show.npz")
    cfg = get_config("show")
    model = _model("bf16", 1.25)
    inp = make_inputs(cfg, int(f["batch"]), seed=int(f["input_seed"]))
    for st, s in (("s100", 1.0), ("s115", 1.15), ("s200", 2.0)):
        model.set_guidance_scale(s)
        eps = _eval(model, inp, int(f["k14_t"]), float(f["k14_c1"]), float(f["k14_c2"]))
        ref = torch.from_numpy(np.concatenate([f[f"k14_{st}_eps_ges"], f[f"k14_{st}_eps_exp"]], axis=-1))
        e, rms = max_abs(eps, ref), float((eps.cpu() - ref).pow(2).mean().sqrt())
        print(f"[guidance bf16 {st}] max|eps-ref| = {e:.3e}, rms = {rms:.3e}")
        assert e < BF16_MAX and rms < BF16_RMS
    model.set_guidance_scale(None)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ddim25_opt_cond_scale_matches_reference(precision):
    f = golden("ddim25_guidance_show.npz")
    cfg = get_config("show")
    model = _model(precision, 1.25)
    B = int(f["batch"])
    inp = make_inputs(cfg, B, seed=int(f["input_seed"]))
    src = SeededNoise(int(f["noise_seed"]))
    opt = sampler_namespace(cfg, cond_scale=float(f["cond_scale"]))
    x, trace = _ddim(model, inp, opt=opt, noise_source=src, return_trace=True, seed=None)
    assert src.count == int(f["draws"]) == 26
    e = rel_err(x, torch.from_numpy(f["final"]))
    print(f"[ddim25 cond_scale {float(f['cond_scale'])} {precision}] rel err {e:.3e}")
    assert e < (REL_TOL if precision == "fp32" else BF16_E2E_REL)
    if precision == "fp32":
        corners = torch.from_numpy(f["step_corner"])
        for i in range(corners.shape[0]):
            assert float((trace[i, :, :3, :6].cpu() - corners[i]).abs().max()) <= REL_TOL * max(float(f["step_stats"][i][2]), 1.0), i
    assert model.guidance_scale is None                      # (opt.cond_scale held for the call only)


# ---- 2. runtime scale == a context created at that scale --------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("created,runtime", [(1.25, 1.15), (1.25, 1.0), (1.0, 1.25)])
def test_runtime_scale_equals_baked_context(precision, created, runtime):
    cfg = get_config("show")
    inp = make_inputs(cfg, 6 if precision == "bf16x3" else 2, seed=3)        # (bf16x3: 528 rows, above the 512-row limit of the split loop)
    _lib.launch_counts(reset=True)
    baked = _model(precision, runtime)
    e_ref = _eval(baked, inp)
    flops_ref = baked.eval_flops()
    x_ref = _ddim(baked, inp)
    model = _model(precision, created)
    _eval(model, inp)                                         # conditioned at its own scale first: the switch must grow / keep the workspace
    model.set_guidance_scale(runtime)
    assert torch.equal(_eval(model, inp), e_ref)
    assert model.eval_flops() == flops_ref
    assert torch.equal(_ddim(model, inp), x_ref)
    model.set_guidance_scale(None)
    if precision == "bf16x3":
        assert_split_ran(_lib.launch_counts(), (created, runtime))


def test_single_transformer_runtime_scale_equals_baked_context():
    cfg = get_config("show", unidiffuser=False)
    inp = make_inputs(cfg, 2, seed=3)
    e_ref, x_ref = _eval(_model("bf16", 1.15, single=True), inp), _ddim(_model("bf16", 1.15, single=True), inp)
    model = _model("bf16", 1.25, single=True)
    model.set_guidance_scale(1.15)
    assert torch.equal(_eval(model, inp), e_ref)
    assert torch.equal(_ddim(model, inp), x_ref)
    model.set_guidance_scale(None)


# ---- 3. per-clip scales, bit for bit --------------------------------------------------------------------------------------
def _per_row_vs_uniform(model, inp, run, scales=MIXED):
    """Row b of the mixed batch == row b of the uniform run at its scale, bit for bit.  A uniform run at 1 is a different model evaluation,
    though: it has no null half, and the first layer's q|k|v is then the folded-LayerNorm launch instead of the LayerNorm row kernel (which
    adds the CFG-null constant) and a plain Linear (denoiser.hip run_block_tail_fused) - the same numbers in another order of operations,
    for every precision.  So rows at 1 are held bit for bit against the same rows of ANOTHER mixed batch that keeps its null half (the
    other clips at 2.0: the same launches, the same row positions), and their distance to the uniform run at 1 is returned (max abs, and
    relative to the range) for the caller to hold under the project's own bar."""
    B = inp["x_T"].shape[0]
    sc = _scales(B, scales)
    model.set_guidance_scale(sc)
    mixed = run()
    at_one = None
    for s in sorted(set(sc)):
        rows = [b for b in range(B) if sc[b] == s]
        if s == 1.0:
            model.set_guidance_scale([1.0 if v == 1.0 else 2.0 for v in sc])
            assert any(v != 1.0 for v in sc) and torch.equal(mixed[rows], run()[rows]), "rows at 1 depend on their neighbours' scales"
        model.set_guidance_scale(s)
        uni = run()
        if s == 1.0:
            at_one = (max_abs(mixed[rows], uni[rows]), rel_err(mixed[rows], uni[rows]))
            continue
        assert torch.equal(mixed[rows], uni[rows]), s
    model.set_guidance_scale(None)
    return at_one


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_per_row_scales_chain_regime(precision):
    """B = 2, T = 88: the window-chain regime (graphs, pipelined two-encoder loop)."""
    model = _model(precision, 1.25)
    inp = make_inputs(model.cfg, 2, seed=3)
    _per_row_vs_uniform(model, inp, lambda: _eval(model, inp))
    _per_row_vs_uniform(model, inp, lambda: _ddim(model, inp))


def test_per_row_scales_mid_size_regime():
    """B = 100: above the graph range, inside the pipelined-loop range."""
    model = _model("bf16", 1.25)
    inp = make_inputs(model.cfg, 100, seed=8)
    _per_row_vs_uniform(model, inp, lambda: _ddim(model, inp))


def test_per_row_scales_sub_batch_streams():
    """B = 950 bf16, one evaluation: three sub-batch instances, each reading its own clips' scales."""
    model = _model("bf16", 1.25)
    inp = make_inputs(model.cfg, 950, seed=9)
    _per_row_vs_uniform(model, inp, lambda: _eval(model, inp))


@pytest.mark.parametrize("regime", ["mid-size loop", "sub-batch streams"])
def test_per_row_scales_on_the_split_loop(regime):
    """precision "bf16x3", B = 100 (8 800 conditional rows), scales 1.0 and 1.25 mixed: the null half of the mixed batch, the CFG-null row
    constant and the FiLM rows are indexed per clip in the split launches.  A ddim25 loop (one batch on the two-encoder pipeline) and one
    evaluation (three sub-batch instances of fp32 storage, each reading its own clips' scales): row b at 1.25 == row b of the uniform run at
    1.25, and row b at 1 == row b of the batch whose other clips run at 2.0, bit for bit.  Rows at 1 against the run WITHOUT a null half
    (half the rows per launch, other tiles, and layer 0's q|k|v in another order of operations: _per_row_vs_uniform) are held under the
    project's unchanged bar, 1e-3 on eps and 1e-3 of the range on a loop; the measured distance is printed."""
    model = _model("bf16x3", 1.25)
    inp = make_inputs(model.cfg, 100, seed=8)
    _lib.launch_counts(reset=True)
    if regime == "mid-size loop":
        d_abs, d_rel = _per_row_vs_uniform(model, inp, lambda: _ddim(model, inp), scales=[1.0, 1.25])
        c = _lib.launch_counts()
        assert (c["sample_streams"], c["sample_graph"], c["sample_pipe"]) == (1, 0, 1), c
        print(f"[measure] guidance bf16x3 B=100 ddim25: rows at scale 1 of the mixed batch vs the run without a null half: {d_rel:.3e} of the range")
        assert d_rel < REL_TOL
    else:
        d_abs, d_rel = _per_row_vs_uniform(model, inp, lambda: _eval(model, inp), scales=[1.0, 1.25])
        c = _lib.launch_counts()
        assert c["eval_streams"] == 3, c
        print(f"[measure] guidance bf16x3 B=100 eval: rows at scale 1 of the mixed batch vs the run without a null half: max |d| = {d_abs:.3e}")
        assert d_abs < FP32_ATOL
    assert_split_ran(c, regime)
    assert c["gemm_f32_split_128"] > 0, c


def test_per_row_scales_masked_window():
    model = _model("bf16", 1.25)
    cfg = model.cfg
    B, L = 4, cfg.overlap_len
    inp = make_inputs(cfg, B, seed=5)
    gt = torch.zeros(B, cfg.n_poses, cfg.net_dim_pose)
    gt[:, :L] = torch.randn(B, L, cfg.net_dim_pose, generator=torch.Generator().manual_seed(17))
    mask = torch.zeros_like(gt, dtype=torch.bool)
    mask[:, :L] = True
    _per_row_vs_uniform(model, inp, lambda: _ddim(model, inp, y={"gt": gt, "outpainting_mask": mask}))


# ---- 4. rows at 1 inside a doubled batch -----------------------------------------------------------------------------------
def test_rows_at_one_match_unguided_oracle():
    _rows_at_one("fp32", [1.0, 1.15, 2.0, 1.0], 32)


def test_rows_at_one_match_unguided_oracle_on_the_split_loop():
    """SHOW B = 6, T = 88 (528 conditional rows, 1 056 with the null half): half_row0 / n_const_rows of the split launches with three of
    the six clips at scale 1."""
    _rows_at_one("bf16x3", [1.0, 1.15, 2.0, 1.0, 1.25, 1.0], 88)


def _rows_at_one(precision, sc, T):
    model = _model(precision, 1.25)
    cfg = model.cfg
    B = len(sc)
    inp = make_inputs(cfg, B, frames=T, seed=12)
    model.set_guidance_scale(sc)
    _lib.launch_counts(reset=True)
    eps = _eval(model, inp, 400, 1.5, 1.1).cpu()
    counts = _lib.launch_counts()
    model.set_guidance_scale(None)
    if precision == "bf16x3":
        assert_split_ran(counts, sc)
    sd = synthetic_sd("show")
    for s in sorted(set(sc)):
        with torch.no_grad():
            ref = denoiser_ref.unidiffuser(sd, dataclasses.replace(cfg, cond_scale=s), inp["x_T"], torch.full((B,), 400), torch.tensor(1.5),
                                           torch.tensor(1.1), inp["audio_emb"], inp["person_id"], inp["pretrain_aud_feat"])
        rows = [b for b in range(B) if sc[b] == s]
        e = max_abs(eps[rows], ref[rows])
        print(f"[mixed batch {precision}, rows at {s}] max|eps - oracle| = {e:.3e}")
        assert e < FP32_ATOL, (s, e)


# ---- 5. chains ------------------------------------------------------------------------------------------------------------------
def test_chains_with_per_chain_scales():
    model = _model("fp32", 1.25)
    cfg = model.cfg
    sc = [1.0, 1.15, 2.0]
    N = cfg.n_poses + 2 * (cfg.n_poses - cfg.overlap_len)           # three windows
    inp = make_inputs(cfg, len(sc), frames=N, seed=14)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    add = {"pretrain_aud_feat": inp["pretrain_aud_feat"]}
    full = tr.sample_arbitrary_len(inp["audio_emb"], inp["person_id"], add, seed=7, row_keys=[0, 1, 2], cond_scale=sc)
    assert full.shape == (3, N, cfg.net_dim_pose)
    for i, s in enumerate(sc):
        one = tr.sample_arbitrary_len(inp["audio_emb"][i:i + 1], inp["person_id"][i:i + 1], {"pretrain_aud_feat": add["pretrain_aud_feat"][i:i + 1]},
                                      seed=7, row_keys=[i], cond_scale=s)
        e = rel_err(full[i:i + 1], one)
        print(f"[chain {i} at {s}] rel err vs alone {e:.3e}")
        assert e < 1e-5
    assert model.guidance_scale is None


def test_sharded_stream_takes_one_scalar():
    model = _model("bf16", 1.25)
    cfg = model.cfg
    N = cfg.n_poses + 3 * (cfg.n_poses - cfg.overlap_len)
    inp = make_inputs(cfg, 1, frames=N, seed=15)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    add = {"pretrain_aud_feat": inp["pretrain_aud_feat"]}
    base = tr.sample_arbitrary_len_sharded(inp["audio_emb"], inp["person_id"], add, 2, seed=3)
    got = tr.sample_arbitrary_len_sharded(inp["audio_emb"], inp["person_id"], add, 2, seed=3, cond_scale=1.15)
    assert model.guidance_scale is None
    model.set_guidance_scale(1.15)
    want = tr.sample_arbitrary_len_sharded(inp["audio_emb"], inp["person_id"], add, 2, seed=3)
    model.set_guidance_scale(None)
    assert torch.equal(got, want) and not torch.equal(got, base)
    with pytest.raises(ValueError):
        tr.sample_arbitrary_len_sharded(inp["audio_emb"], inp["person_id"], add, 2, seed=3, cond_scale=[1.15, 2.0])


# ---- 6. interface ---------------------------------------------------------------------------------------------------------------
def test_set_none_restores_config_value():
    model = _model("fp32", 1.25)
    inp = make_inputs(model.cfg, 2, frames=24, seed=1)
    base = _eval(model, inp)
    model.set_guidance_scale(2.0)
    assert model.guidance_scale == (2.0,)
    assert not torch.equal(_eval(model, inp), base)
    model.set_guidance_scale(None)
    assert model.guidance_scale is None
    assert torch.equal(_eval(model, inp), base)


def test_loop_keyword_wins_over_opt_and_is_restored(monkeypatch):
    model = _model("fp32", 1.25)
    cfg = model.cfg
    inp = make_inputs(cfg, 2, frames=24, seed=2)
    model.set_guidance_scale(1.15)
    want = _ddim(model, inp)
    model.set_guidance_scale(2.0)
    got = _ddim(model, inp, opt=sampler_namespace(cfg, cond_scale=0.5), cond_scale=1.15)
    assert torch.equal(got, want)
    assert model.guidance_scale == (2.0,)
    at2 = _ddim(model, inp)
    # ... also when the native loop fails
    lib = _lib.lib()
    monkeypatch.setattr(lib, "dsh_sample_run", lambda *a: -1)
    with pytest.raises(_lib.DshError):
        _ddim(model, inp, cond_scale=1.15)
    monkeypatch.undo()
    assert model.guidance_scale == (2.0,)
    assert torch.equal(_ddim(model, inp), at2)
    model.set_guidance_scale(None)


def test_bad_scales_raise():
    model = _model("fp32", 1.25)
    inp = make_inputs(model.cfg, 2, frames=24, seed=4)
    _eval(model, inp)
    with pytest.raises(ValueError):
        model.set_guidance_scale(float("nan"))
    with pytest.raises(ValueError):
        _ddim(model, inp, cond_scale=[1.1, 1.2, 1.3])                 # wrong length for B = 2
    model.set_guidance_scale([1.1, 1.2, 1.3])                           # sticky: checked against the batch when it runs
    with pytest.raises(_lib.DshError):
        _eval(model, inp)
    model.set_guidance_scale(None)
    lib = _lib.lib()
    nan = (C.c_float * 1)(float("nan"))
    assert lib.dsh_set_guidance_scale(model._h, nan, 1) == -1
    assert model.guidance_scale is None
    _eval(model, inp)


def test_beat_non_cfg_weights():
    cfg = get_config("beat")
    model = _model("fp32", 1.0, ds="beat")
    inp = make_inputs(cfg, 2, seed=3)
    with pytest.raises(ValueError):
        model.set_guidance_scale(1.15)
    with pytest.raises(ValueError):
        _ddim(model, inp, cond_scale=1.15)
    lib = _lib.lib()
    assert lib.dsh_set_guidance_scale(model._h, (C.c_float * 1)(1.15), 1) == -1
    model.set_guidance_scale(1.0)                                       # 1 is fine
    model.set_guidance_scale(None)
    base = _ddim(model, inp)
    ignored = _ddim(model, inp, opt=sampler_namespace(cfg, cond_scale=1.15))   # the reference never reads it without CFG weights
    assert torch.equal(base, ignored)
