"""One modality alone on a real MI355X (UniDiffuser.set_condition(modality=, expression=), dsh_set_modality): expression-only, and
gestures for a given expression track.

  * expression mode: the expression columns of every evaluation and loop are the joint run's, bit for bit, the gesture columns 0;
  * gesture mode given the joint evaluation's own expression estimate (debug tap): the gesture columns are the joint run's, bit for bit;
  * gesture loops against the CPU composition (tests/modality_ref.py) and the imported reference's fixtures (tests/golden/modality_*.npz);
  * the inactive columns of x / gt / noise are never read; chains; lifetime and refusals; work really removed; the sharded path.

The regime shapes (SHOW, T = 88): B = 2 (graph / pipeline range), B = 141 (12 408 rows: plain evaluations split over two sub-batch
streams, loops unsplit), B = 734 (64 592 rows: loops split over three sub-batch streams; 3-step DDIM).  precision "bf16x3" (the fp32 path with its Linears of more
than 512 rows on the split-bf16 loop) runs at B = 6 (528 rows, the smallest batch above the limit) and B = 141 (three sub-batch streams): the
concat segments of feat_proj.1 change under a modality, and every bit-equality of the fp32 path must hold on the split loop too.  The models are private to this
module (the session-wide handles of tests/util.py keep their own sticky settings)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import modality_ref as M  # noqa: E402
from diffsheg_amd import _lib  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.diffusion import ModelMeanType, ModelVarType, SpacedDiffusion, get_named_beta_schedule, space_timesteps  # noqa: E402
from diffsheg_amd.model import MotionTransformer, UniDiffuser  # noqa: E402
from diffsheg_amd.synthetic import SeededNoise, make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace, sample_arbitrary_len_sharded, window_seed  # noqa: E402
from diffsheg_amd.weights import make_synthetic_state_dict  # noqa: E402
from oracle import sampler_ref  # noqa: E402
from util import assert_split_ran, rel_err, synthetic_sd  # noqa: E402

LOOP_GATE = {"fp32": 1e-3, "bf16": 1.2e-2}       # of the output range: the project's loop gate (test_gpu_sampler) / bf16 end-to-end gate
SHARD_GATE = {"fp32": 1e-5, "bf16": 0.0}         # a chain alone vs its row of the batched run: bit-identical in bf16, 1e-5 of range in fp32
SHARDED_FILE_GATE = {"fp32": 1e-5, "bf16": 1.2e-2}   # tests/test_gpu_sharded.py's gate of the sharded stream against chains sampled alone
REGIMES = [2, 141, 734]

_MODELS = {}


def _model(precision="fp32", ds="show", single=False):
    key = (ds, precision, single)
    if key not in _MODELS:
        cfg = get_config(ds, unidiffuser=not single)
        cls = MotionTransformer if single else UniDiffuser
        sd = make_synthetic_state_dict(cfg, 1234) if single else synthetic_sd(ds)
        _MODELS[key] = cls(cfg, sd, device="cuda:0", precision=precision)
    m = _MODELS[key]
    m.set_guidance_scale(None)
    return m


@functools.lru_cache(maxsize=8)
def _inputs(ds, B, T=None, seed=31):
    """Device inputs of a batch: 64 seeded clips repeated, every clip made distinct by a per-clip offset of its mel features."""
    cfg = get_config(ds)
    small = make_inputs(cfg, min(B, 64), frames=T, seed=seed)
    rep = (B + 63) // 64
    out = {k: v.repeat(rep, *([1] * (v.dim() - 1)))[:B].cuda().contiguous() for k, v in small.items()}
    out["audio_emb"] += 1e-3 * torch.arange(B, device="cuda:0", dtype=torch.float32).view(B, 1, 1)
    out["x_T"] += 1e-3 * torch.arange(B, device="cuda:0", dtype=torch.float32).view(B, 1, 1)
    pid = torch.zeros(B, cfg.style_dim, device="cuda:0")
    pid[torch.arange(B), torch.arange(B) % cfg.style_dim] = 1.0
    out["person_id"] = pid
    return out


def _kw(inp, y=None, lengths=None, modality=None, expression=None):
    kw = {"audio_emb": inp["audio_emb"], "length": None if lengths is None else torch.tensor(lengths), "person_id": inp["person_id"],
          "add_cond": {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "y": {} if y is None else y, "pe_type": "pe_sinu"}
    if modality is not None:
        kw["modality"], kw["expression"] = modality, expression
    return kw


def _eval(model, inp, modality="both", expression=None, lengths=None, x=None, t=560, c1=4.9, c2=4.8):
    cfg = model.cfg
    x = inp["x_T"] if x is None else x
    B, T = x.shape[:2]
    shape_e = (B, T, cfg.expression_dim)
    return model(x, torch.full((B,), t, dtype=torch.long).cuda(), sqrt_alphas=[torch.full(shape_e, float(c1)), torch.full(shape_e, float(c2))],
                 audio_emb=inp["audio_emb"], length=None if lengths is None else torch.tensor(lengths), person_id=inp["person_id"],
                 add_cond={"pretrain_aud_feat": inp["pretrain_aud_feat"]}, pe_type="pe_sinu", y={}, modality=modality, expression=expression)


@functools.lru_cache(maxsize=4)
def _ddim3(ds):
    cfg = get_config(ds)
    return SpacedDiffusion(use_timesteps=space_timesteps(cfg.diffusion_steps, "ddim3"), rescale_timesteps=False, opt=sampler_namespace(cfg),
                           betas=get_named_beta_schedule("linear", cfg.diffusion_steps), model_mean_type=ModelMeanType.EPSILON,
                           model_var_type=ModelVarType.FIXED_SMALL, loss_type=None)


def _loop(model, inp, loop="ddim25", y=None, lengths=None, modality=None, expression=None, **kw):
    """One sampling loop: ddim25 / ddim3 / ddim25 at eta = 0.5 / the 50-step DDPM loop."""
    cfg = model.cfg
    B, T = inp["audio_emb"].shape[:2]
    shape, mk = (B, T, cfg.net_dim_pose), _kw(inp, y, lengths, modality, expression)
    if loop == "ddpm50":
        tr = DDPMTrainer(sampler_namespace(cfg, ddim=False, diffusion_steps=50), model)
        return tr.diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs=mk, **kw)
    if loop == "ddim3":
        return _ddim3(cfg.dataset).ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=mk, **kw)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    return tr.diffusion_ddim_val.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=mk, eta=0.5 if loop == "eta05" else 0.0, **kw)


def _masked_y(cfg, B, T, seed=17):
    """A chain's second window: the first overlap_len frames pinned."""
    L = cfg.overlap_len
    g = torch.Generator().manual_seed(seed)
    gt = torch.zeros(B, T, cfg.net_dim_pose)
    gt[:, :L] = torch.randn(min(B, 8), L, cfg.net_dim_pose, generator=g).repeat((B + 7) // 8, 1, 1)[:B]
    mask = torch.zeros(B, T, cfg.net_dim_pose, dtype=torch.bool)
    mask[:, :L] = True
    return {"gt": gt.cuda(), "outpainting_mask": mask.cuda(), "outpainting_mask_any": True}


class _DeviceNoise:
    """Injected noise stack drawn on the device (a seeded generator): the same draws for every run built with the same seed."""

    def __init__(self, seed):
        self.gen = torch.Generator(device="cuda:0").manual_seed(seed)

    def randn(self, shape):
        return torch.randn(*shape, device="cuda:0", generator=self.gen)


def _setting(model, B, setting):
    """Per-clip guidance scales (1.0, 1.25) / ragged lengths (88, 40) of the evaluation tests -> lengths."""
    T = model.cfg.n_poses
    if setting == "scales":
        model.set_guidance_scale([(1.0, 1.25)[b % 2] for b in range(B)])
    return [(T, 40)[b % 2] for b in range(B)] if setting == "ragged" else None


def _valid(out, lengths):
    """Frames of a ragged evaluation that are defined (padded output frames are unspecified)."""
    if lengths is None:
        return out
    return torch.cat([out[b, :n].reshape(-1) for b, n in enumerate(lengths)])


EVAL_CASES = [(p, B, "plain") for p in ("fp32", "bf16") for B in REGIMES] + [(p, 2, s) for p in ("fp32", "bf16") for s in ("scales", "ragged")] + \
             [("bf16", 141, "scales"), ("bf16", 141, "ragged")] + \
             [("bf16x3", 6, "plain"), ("bf16x3", 6, "scales"), ("bf16x3", 6, "ragged"), ("bf16x3", 141, "plain")]


# ---- 1. expression evaluation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,B,setting", EVAL_CASES)
def test_expression_evaluation_is_the_joint_evaluation(precision, B, setting):
    model = _model(precision)
    G = model.cfg.split_pos
    inp = _inputs("show", B)
    lengths = _setting(model, B, setting)
    _lib.launch_counts(reset=True)
    joint = _eval(model, inp, lengths=lengths).clone()
    torch.cuda.synchronize()
    jc = _lib.launch_counts(reset=True)
    streams = jc["eval_streams"]
    part = _eval(model, inp, "expression", lengths=lengths)
    torch.cuda.synchronize()
    model.set_guidance_scale(None)
    if precision == "bf16x3":
        assert_split_ran(jc, "joint")
        assert_split_ran(_lib.launch_counts(), "expression")
    # (the regime is the joint run's — bf16: one stream, two from 12 288 token rows, three from 64 500; fp32: two from 4 096, three from 8 700)
    assert _lib.launch_counts()["eval_streams"] == streams == {2: 1, 6: 1, 141: 2 if precision == "bf16" else 3, 734: 3}[B]
    assert torch.equal(_valid(part[..., G:], lengths), _valid(joint[..., G:], lengths))
    assert not part[..., :G].any()
    assert joint[..., :G].abs().max() > 0


# ---- 2. gesture evaluation given the joint run's own expression estimate ------------------------------------------------------------------
@pytest.mark.parametrize("precision,B,setting", EVAL_CASES)
def test_gesture_evaluation_given_the_joint_estimate_is_the_joint_evaluation(precision, B, setting):
    model = _model(precision)
    G = model.cfg.split_pos
    inp = _inputs("show", B)
    lengths = _setting(model, B, setting)
    joint = _eval(model, inp, lengths=lengths).clone()
    tap = model.debug_tap("expr_x0").clone()
    _lib.launch_counts(reset=True)
    part = _eval(model, inp, "gesture", tap, lengths=lengths)
    model.set_guidance_scale(None)
    if precision == "bf16x3":
        assert_split_ran(_lib.launch_counts(), "gesture")
    assert torch.equal(_valid(part[..., :G], lengths), _valid(joint[..., :G], lengths))
    assert not part[..., G:].any()


# ---- 3. expression loops ------------------------------------------------------------------------------------------------------------------
def _noise_kw(noise, B, T, Cc, seed=4321):
    if noise == "stack":
        return lambda: {"noise_source": _DeviceNoise(seed)}, None
    if noise == "philox":
        return lambda: {"seed": seed}, None
    lengths = [(T, 40)[b % 2] for b in range(B)]                 # row keys with ragged lengths (40 * C is a multiple of 4)
    return lambda: {"seed": seed, "row_keys": list(range(500, 500 + B))}, lengths


LOOP_CASES = [("fp32", 2, lp, "stack") for lp in ("ddim25", "masked", "eta05", "ddpm50")] + \
             [("bf16", 2, lp, nz) for lp in ("ddim25", "masked") for nz in ("stack", "philox", "rows")] + [("bf16", 2, "eta05", "rows"), ("bf16", 2, "ddpm50", "philox")] + \
             [("bf16", 141, "ddim25", "stack"), ("bf16", 141, "masked", "rows"), ("bf16", 141, "eta05", "philox"), ("bf16", 141, "ddpm50", "philox"),
              ("fp32", 141, "ddim25", "philox")] + \
             [("bf16", 734, "ddim3", nz) for nz in ("stack", "philox", "rows")] + [("bf16", 734, "ddim3_masked", "philox"), ("bf16", 734, "ddim3_eta05", "rows"),
              ("bf16", 734, "masked", "philox")] + \
             [("bf16x3", 6, "ddim25", "philox"), ("bf16x3", 6, "masked", "rows"), ("bf16x3", 141, "ddim25", "philox")]
# (bf16 734 masked: the ddim25 jump schedule on sub-batch streams - the inline timestep cache, each instance its active share)


@pytest.mark.parametrize("precision,B,loop,noise", LOOP_CASES)
def test_expression_loop_is_the_joint_loop(precision, B, loop, noise):
    model = _model(precision)
    cfg = model.cfg
    G, T, Cc = cfg.split_pos, cfg.n_poses, cfg.net_dim_pose
    inp = _inputs("show", B)
    y = _masked_y(cfg, B, T) if "masked" in loop else None
    kind = "ddim3" if loop.startswith("ddim3") else ("ddim25" if loop == "masked" else loop)
    extra = {"eta": 0.5} if loop == "ddim3_eta05" else {}
    nkw, lengths = _noise_kw(noise, B, T, Cc)
    _lib.launch_counts(reset=True)
    joint = _loop(model, inp, kind, y, lengths, **nkw(), **extra).clone()
    torch.cuda.synchronize()
    jc = _lib.launch_counts(reset=True)
    part = _loop(model, inp, kind, y, lengths, "expression", **nkw(), **extra)
    torch.cuda.synchronize()
    pc = _lib.launch_counts()
    # the regime is the joint run's (graphs at B = 2, one batch below 64 500 token rows, three sub-batch streams above); the joint loop below the
    # split runs its two encoders as a two-stream pipeline, the partial loop is one chain
    assert (pc["sample_graph"], pc["sample_streams"]) == (jc["sample_graph"], jc["sample_streams"]) == ({2: 1, 6: 1, 141: 0, 734: 0}[B], {2: 1, 6: 1, 141: 1, 734: 3}[B])
    assert jc["sample_pipe"] == (1 if B < 734 else 0) and pc["sample_pipe"] == 0
    if precision == "bf16x3":
        assert_split_ran(jc, "joint loop")
        assert_split_ran(pc, "expression loop")
    assert torch.isfinite(joint).all() and joint[..., G:].abs().max() > 0
    assert torch.equal(part[..., G:], joint[..., G:])
    assert not part[..., :G].any()


# ---- 4. gesture loops against the composition and the reference fixtures -----------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("ds", ["show", "beat"])
def test_gesture_loops_match_composition_and_reference(ds, precision):
    """SHOW B = 2 (T = 88), BEAT B = 3 (T = 34): a plain ddim25 loop and one out-painting window, gestures for a seeded given track.
    Measured on MI355X (max error / output range; fixture, composition): see DESIGN.md §2."""
    c = M.fixture_case(ds)
    cfg, f, G, track = c["cfg"], c["f"], c["cfg"].split_pos, c["track"]
    model = _model(precision, ds)
    tr_dev = track.cuda()
    runs = (("ddim", c["inp"], None, int(f["noise_seed"]), c["comp_ddim"]),
            ("masked", c["inp_m"], {k: v.cuda() for k, v in c["y"].items()}, int(f["masked_noise_seed"]), c["comp_masked"]))
    for name, inp, y, nseed, comp in runs:
        dev = {k: v.cuda() for k, v in inp.items()}
        x = _loop(model, dev, "ddim25", y, None, "gesture", tr_dev, noise_source=SeededNoise(nseed)).cpu()
        ref = torch.from_numpy(f[f"{name}_final_ges"])
        e_ref, e_comp = rel_err(x[..., :G], ref), rel_err(x[..., :G], comp[..., :G])
        print(f"[modality {ds} {precision} gesture {name}] err / range: vs reference fixture {e_ref:.3e}, vs composition {e_comp:.3e}")
        assert e_ref < LOOP_GATE[precision] and e_comp < LOOP_GATE[precision], (name, e_ref, e_comp)
        assert torch.equal(x[..., G:], track)                     # the expression columns of the result are the given track, bit for bit


# ---- 5. inactive inputs are never read ---------------------------------------------------------------------------------------------------
class _GarbageNoise(_DeviceNoise):
    """The same draws, with the columns [lo, hi) of every one replaced by finite garbage."""

    def __init__(self, seed, lo, hi, fill):
        super().__init__(seed)
        self.lo, self.hi, self.fill = lo, hi, fill

    def randn(self, shape):
        z = super().randn(shape)
        if self.fill is not None:
            z[..., self.lo:self.hi] = self.fill
        return z


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("modality", ["expression", "gesture"])
def test_inactive_inputs_are_never_read(modality, precision):
    model = _model(precision)
    cfg = model.cfg
    G, T, Cc, B = cfg.split_pos, cfg.n_poses, cfg.net_dim_pose, 6 if precision == "bf16x3" else 2      # (bf16x3: above the 512-row limit)
    _lib.launch_counts(reset=True)
    lo, hi = (0, G) if modality == "expression" else (G, Cc)       # the inactive columns
    inp = _inputs("show", B)
    track = M.make_track(cfg, B, 5).cuda() if modality == "gesture" else None
    y = _masked_y(cfg, B, T)

    def dirty(t, v):
        t = t.clone()
        t[..., lo:hi] = v
        return t
    # evaluation: x
    clean = _eval(model, inp, modality, track).clone()
    assert torch.equal(_eval(model, inp, modality, track, x=dirty(inp["x_T"], 123.0)), clean)
    # out-painting loop started from a given x: x, gt and every draw of the noise stack
    x0 = inp["x_T"]
    want = _loop(model, inp, "ddim25", y, None, modality, track, noise=x0, noise_source=_GarbageNoise(9, lo, hi, None)).clone()
    y2 = dict(y, gt=dirty(y["gt"], -77.0))
    got = _loop(model, inp, "ddim25", y2, None, modality, track, noise=dirty(x0, 1e4), noise_source=_GarbageNoise(9, lo, hi, 55.5))
    assert torch.equal(got, want)
    # plain loop whose x_T is the first draw
    want = _loop(model, inp, "ddim25", None, None, modality, track, noise_source=_GarbageNoise(9, lo, hi, None)).clone()
    got = _loop(model, inp, "ddim25", None, None, modality, track, noise_source=_GarbageNoise(9, lo, hi, -3e3))
    assert torch.equal(got, want)
    if precision == "bf16x3":
        assert_split_ran(_lib.launch_counts(), modality)


# ---- 6. chains -----------------------------------------------------------------------------------------------------------------------------
def _stream(ds, B, N, seed=41):
    cfg = get_config(ds)
    inp = make_inputs(cfg, B, frames=N, seed=seed)
    return cfg, inp["audio_emb"].cuda(), inp["pretrain_aud_feat"].cuda(), inp["person_id"].cuda()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_expression_chain_is_the_joint_chain(precision):
    """3 windows including a short tail (BEAT: n_poses 34)."""
    model = _model(precision, "beat")
    cfg, a, h, p = _stream("beat", 2, 2 * (34 - get_config("beat").overlap_len) + 34 - 9)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    G = cfg.split_pos
    assert len(M.sr.get_windows(a, cfg.n_poses, cfg.n_poses - cfg.overlap_len)) == 3
    joint = tr.sample_arbitrary_len(a, p, {"pretrain_aud_feat": h}, seed=7, row_keys=[3, 4]).clone()
    part = tr.sample_arbitrary_len(a, p, {"pretrain_aud_feat": h}, seed=7, row_keys=[3, 4], modality="expression")
    assert torch.equal(part[..., G:], joint[..., G:]) and not part[..., :G].any()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_gesture_chain_matches_the_composition(precision):
    """One BEAT chain of 3 windows (short tail) with an [N, E] track, injected noise per window."""
    model = _model(precision, "beat")
    cfg = get_config("beat")
    N = 2 * (cfg.n_poses - cfg.overlap_len) + cfg.n_poses - 9
    _, a, h, p = _stream("beat", 1, N)
    track = M.make_track(cfg, 1, 6, frames=N)[0]                                    # [N, E]
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    G = cfg.split_pos
    x = tr.sample_arbitrary_len(a, p, {"pretrain_aud_feat": h}, noise_source_for_window=lambda i: SeededNoise(60 + i), modality="gesture",
                                expression=track).cpu()
    with torch.no_grad():
        comp = M.window_chain(synthetic_sd("beat"), cfg, a.cpu(), p.cpu(), h.cpu(), track.unsqueeze(0), lambda i: sampler_ref.NoiseSource(seed=60 + i))
    e = rel_err(x[..., :G], comp[..., :G])
    print(f"[modality beat {precision} gesture chain] err / range vs composition {e:.3e}")
    assert e < LOOP_GATE[precision]
    assert torch.equal(x[0, :, G:], track)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_gesture_chains_alone_equal_their_rows_and_lengths_form(precision):
    model = _model(precision, "beat")
    cfg = get_config("beat")
    step = cfg.n_poses - cfg.overlap_len
    N = 2 * step + cfg.n_poses - 9
    _, a, h, p = _stream("beat", 2, N)
    track = M.make_track(cfg, 2, 8, frames=N).cuda()
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    G, cnd = cfg.split_pos, {"pretrain_aud_feat": h}
    both = tr.sample_arbitrary_len(a, p, cnd, seed=7, row_keys=[11, 12], modality="gesture", expression=track).clone()
    assert torch.equal(both[..., G:], track)
    for b, key in enumerate([11, 12]):
        solo = tr.sample_arbitrary_len(a[b:b + 1], p[b:b + 1], {"pretrain_aud_feat": h[b:b + 1]}, seed=7, row_keys=[key], modality="gesture",
                                       expression=track[b:b + 1])
        e = rel_err(solo[0], both[b])
        print(f"[modality beat {precision}] gesture chain {b} alone vs its row of the batch: {e:.3e}")
        assert e <= SHARD_GATE[precision]
    # the lengths= form: two chains of different lengths, the track as a list; the full-length chain is the chain above
    lens = [N, N - step - 5]
    outs = tr.sample_arbitrary_len(a, p, cnd, seed=7, row_keys=[11, 12], lengths=lens, modality="gesture", expression=[track[0, :lens[0]], track[1, :lens[1]]])
    assert [tuple(o.shape) for o in outs] == [(n, cfg.net_dim_pose) for n in lens]
    for b in range(2):
        assert torch.equal(outs[b][:, G:], track[b, :lens[b]])
        assert torch.isfinite(outs[b]).all() and outs[b][:, :G].abs().max() > 0
    assert rel_err(outs[0], both[0]) <= SHARD_GATE[precision]


# ---- 7. lifetime and refusals ------------------------------------------------------------------------------------------------------------
def test_lifetime_and_refusals():
    cfg, sd = get_config("show"), synthetic_sd("show")
    B, T = 2, cfg.n_poses
    inp = _inputs("show", B)
    track = M.make_track(cfg, B, 5).cuda()
    fresh = UniDiffuser(cfg, sd, device="cuda:0", precision="bf16")
    want_eval = _eval(fresh, inp).clone()
    want_loop = _loop(fresh, inp, seed=5).clone()
    del fresh
    model = UniDiffuser(cfg, sd, device="cuda:0", precision="bf16")
    lib = _lib.lib()

    def joint_unchanged():
        assert torch.equal(_eval(model, inp), want_eval)
        assert torch.equal(_loop(model, inp, seed=5), want_loop)

    # after partial runs, set_condition + a joint call = a fresh context
    _eval(model, inp, "gesture", track)
    _loop(model, inp, modality="gesture", expression=track, seed=5)
    _loop(model, inp, modality="expression", seed=5)
    assert model.modality == 1
    joint_unchanged()
    assert model.modality == 0
    # Python refusals (ValueError, before anything is conditioned)
    for kw in (dict(modality="gesture"), dict(modality="gesture", expression=track[:, :-1]), dict(modality="face"), dict(modality=7),
               dict(modality="expression", expression=track)):
        with pytest.raises(ValueError):
            _eval(model, inp, **kw)
        with pytest.raises(ValueError):
            model.set_condition(inp["audio_emb"], inp["person_id"], inp["pretrain_aud_feat"], **kw)
        joint_unchanged()
    son = DDPMTrainer(sampler_namespace(cfg, same_overlap_noisy=True), model)
    with pytest.raises(ValueError, match="same_overlap_noisy"):
        son.generate_batch(inp["audio_emb"], inp["person_id"], cfg.net_dim_pose, {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, {"clip_idx": 0},
                           seed=5, modality="expression")
    joint_unchanged()
    with pytest.raises(ValueError):
        DDPMTrainer(sampler_namespace(cfg), model).validate_batch(inp["audio_emb"], inp["x_T"], inp["person_id"],
                                                                   {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, modality="expression")
    # the C interface: -1 with dsh_last_error, the condition stays usable
    _eval(model, inp)
    for mod, ptr in ((5, None), (-1, None), (2, None)):
        assert lib.dsh_set_modality(model._h, mod, ptr) == -1 and lib.dsh_last_error()
    torch.cuda.synchronize()
    joint_unchanged()
    # same_overlap_noisy together with a partial modality: dsh_sample refuses, the modality of the condition stays usable
    model.set_condition(inp["audio_emb"], inp["person_id"], inp["pretrain_aud_feat"], modality="expression")
    opts = son.diffusion_ddim_val._opts(0, False, 1, 5)
    x = torch.zeros(B, T, cfg.net_dim_pose, device="cuda:0")
    assert lib.dsh_sample(model._h, C.byref(opts), x.data_ptr(), 0, None, None, 0, None, 0, None) == -1
    assert b"same_overlap_noisy" in lib.dsh_last_error()
    torch.cuda.synchronize()
    model._cond_key = None
    joint_unchanged()
    # a single-MotionTransformer context
    single = _model("bf16", single=True)
    with pytest.raises(ValueError, match="MotionTransformer"):
        single.set_condition(inp["audio_emb"], inp["person_id"], inp["pretrain_aud_feat"], modality="expression")
    single.set_condition(inp["audio_emb"], inp["person_id"], inp["pretrain_aud_feat"])
    assert lib.dsh_set_modality(single._h, 1, None) == -1
    assert lib.dsh_set_modality(single._h, 0, None) == 0
    # before any condition
    bare = UniDiffuser(cfg, sd, device="cuda:0", precision="bf16")
    assert lib.dsh_set_modality(bare._h, 1, None) == -1
    del bare, model


# ---- 8. work really removed ----------------------------------------------------------------------------------------------------------------
def _profile(model, fn):
    lib = _lib.lib()
    _lib.check(lib.dsh_profile_enable(model._h, 1))
    fn()
    ms = (C.c_double * 16)(); n = (C.c_int64 * 16)(); fl = (C.c_double * 16)(); by = (C.c_double * 16)()
    _lib.check(lib.dsh_profile_read(model._h, ms, n, fl, by))
    _lib.check(lib.dsh_profile_enable(model._h, 0))
    return [int(v) for v in n]


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
def test_work_is_really_removed(precision):
    model = _model(precision)
    B = 6 if precision == "bf16x3" else 2                          # (bf16x3: above the 512-row limit)
    inp = _inputs("show", B)
    track = M.make_track(model.cfg, B, 5).cuda()
    flops, launches = {}, {}
    for mod, ex in (("both", None), ("expression", None), ("gesture", track)):
        _lib.launch_counts(reset=True)
        _eval(model, inp, mod, ex)
        if precision == "bf16x3":
            assert_split_ran(_lib.launch_counts(), mod)
        flops[mod] = model.eval_flops()
        model._cond_key = None                                     # (the profiler changes the split decision: condition again under it)
        launches[mod] = _profile(model, lambda: _eval(model, inp, mod, ex))
        model._cond_key = None
    print(f"[modality {precision}] eval flops {flops}; profiled launches {({k: sum(v) for k, v in launches.items()})}")
    assert 0 < flops["expression"] < flops["both"] and 0 < flops["gesture"] < flops["both"]
    assert flops["expression"] + flops["gesture"] >= flops["both"]          # (the shared head is counted once in each partial figure)
    assert sum(launches["expression"]) < sum(launches["both"]) and sum(launches["gesture"]) < sum(launches["both"])
    # classes that only the gesture encoder's concat form uses: nothing of them in an expression-only run
    lib = _lib.lib()
    only_ges = []
    for c in range(16):
        kn, rl = C.c_char_p(), C.c_char_p()
        _lib.check(lib.dsh_profile_class_info(model._h, c, C.byref(kn), C.byref(rl)))
        if rl.value and rl.value.decode().startswith("gesture encoder"):
            only_ges.append(c)
    assert only_ges
    for c in only_ges:
        assert launches["expression"][c] == 0
        if precision == "bf16":
            assert launches["both"][c] == model.cfg.num_layers == launches["gesture"][c]


# ---- 9. sharded path -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sharded_gesture_stream_equals_the_unsharded_chains(precision):
    """World size 1: chains + seam repair through the sharded entry point == the same chains and seam window sampled directly."""
    model = _model(precision, "beat")
    cfg = get_config("beat")
    n_poses, L, G = cfg.n_poses, cfg.overlap_len, cfg.split_pos
    step = n_poses - L
    N = 4 * step + L                                               # two segments of two strides
    _, a, h, p = _stream("beat", 1, N, seed=43)
    track = M.make_track(cfg, 1, 10, frames=N).cuda()
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    out = sample_arbitrary_len_sharded(tr, a, p, {"pretrain_aud_feat": h}, n_segments=2, seed=21, seam_repair=True, modality="gesture",
                                       expression=track).clone()
    assert out.shape == (1, N, cfg.net_dim_pose)
    assert torch.equal(out[..., G:], track)
    from diffsheg_amd.trainer import SEAM_WINDOW, seam_windows, split_segments_for_repair
    segs = split_segments_for_repair(N, 2, n_poses, L)
    assert len(segs) == 2
    parts = []
    for i, sg in enumerate(segs):
        sl = slice(sg.start, sg.stop)
        parts.append(tr.sample_arbitrary_len(a[:, sl], p, {"pretrain_aud_feat": h[:, sl]}, seed=21, row_keys=[i], modality="gesture",
                                             expression=track[:, sl])[0])
    ref = torch.cat(parts, 0)
    w = seam_windows(segs, n_poses)[0]
    ws = slice(w.start, w.stop)
    win = ref[ws].unsqueeze(0)
    ref[ws] = tr.sample_inbetween(a[:, ws], p, {"pretrain_aud_feat": h[:, ws]}, win[:, :L], win[:, n_poses - L:], seed=window_seed(21, SEAM_WINDOW),
                                  row_keys=[0], modality="gesture", expression=track[:, ws].contiguous())[0]
    e = rel_err(out[0], ref)
    print(f"[modality beat {precision}] sharded gesture stream vs the unsharded calls: {e:.3e}")
    assert e <= SHARDED_FILE_GATE[precision]
