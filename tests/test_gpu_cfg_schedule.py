"""Guidance schedules on a real MI355X (dsh_set_guidance_schedule, UniDiffuser.set_guidance_schedule, cfg_schedule= of the loops,
glue.CFGSchedule): the scheduled mix and the std rescale one launch at a time against the emulation of cfg_schedule_ref.py, and the model
with SHOW synthetic weights — trivial schedules against the unscheduled bits, gains against uniform runs at the effective scale, the
oracle composed per encoder on the CPU, every loop regime against the single-stream eager loop, and the argument rules.

The models here are private to this module (a schedule is sticky in its context)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cfg_schedule_ref as S  # noqa: E402
import small_ops_ref as R  # noqa: E402
from diffsheg_amd import _lib  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.glue import CFGSchedule  # noqa: E402
from diffsheg_amd.model import MotionTransformer, UniDiffuser  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from diffsheg_amd.weights import make_synthetic_state_dict  # noqa: E402
from oracle import denoiser_ref  # noqa: E402
from util import assert_split_ran, max_abs, synthetic_sd  # noqa: E402

DEV = "cuda:0"
FP32_ATOL = 1e-3                       # test_gpu_eval's golden tolerance
BF16_MAX, BF16_RMS = 6e-2, 1.5e-2      # test_gpu_eval's bf16 gates
ULPS = 2                               # rescaled elements: f is rounded once from fp64 sums taken in another order (<= 1 ulp), the product once more


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ============================================================ op level ============================================================
def _guarded(shape):
    n = int(np.prod(shape))
    return torch.full((n + R.GUARD,), R.SENTINEL, dtype=torch.float32).to(DEV)


def _split(buf, shape):
    n = int(np.prod(shape))
    h = buf.cpu()
    assert bool((h[n:] == R.SENTINEL).all()), "guard behind the buffer overwritten"
    return h[:n].reshape(shape)


def _op(t, x0_on=True, nan_pad=False):
    """dsh_op_cfg_mix_sched on the emulation's inputs -> (eps columns [c0, c0 + w), x0 [Mc, w] or None) on the CPU; everything the launch
    must not write (pad columns, the guard) is checked here"""
    Mc, w, c0, T = t["Mc"], t["w"], t["c0"], t["T"]
    o = t["o"].clone()
    if nan_pad:
        for b, n in enumerate(t["lens"]):
            for half in (0, t["cond_row0"]):
                o[half + b * T + n:half + (b + 1) * T] = float("nan")
    d = {n: t[n].to(DEV) for n in ("x", "scale", "c1", "c2", "t", "table")}
    od = o.to(DEV)
    lens = None if t["lens"] is None else torch.tensor(t["lens"], dtype=torch.int32, device=DEV)
    eps = _guarded((Mc, t["lde"]))
    x0 = _guarded((Mc, t["ldx0"])) if x0_on else None
    _lib.check(_lib.lib().dsh_op_cfg_mix_sched(None, _p(od), t["ldo"], Mc, t["cond_row0"], T, w, 1, _p(d["scale"]), t["scale_row"], _p(eps), t["lde"], c0,
                                              _p(d["x"]), t["ldx"], _p(d["c1"]), _p(d["c2"]), _p(x0), t["ldx0"], _p(d["t"]), t["t_row"], _p(d["table"]),
                                              int(t["table"].shape[1]), t["which"], t["phi"], _p(lens)), "dsh_op_cfg_mix_sched")
    torch.cuda.synchronize()
    e = _split(eps, (Mc, t["lde"]))
    assert bool((e[:, :c0] == R.SENTINEL).all()) and bool((e[:, c0 + w:] == R.SENTINEL).all()), "eps: a column outside [c0, c0 + w) written"
    e = e[:, c0:c0 + w].contiguous()
    if not x0_on:
        return e, None
    z = _split(x0, (Mc, t["ldx0"]))
    assert bool((z[:, w:] == R.SENTINEL).all()), "x0: a pad column written"
    return e, z[:, :w].contiguous()


OP_SHAPES = [(w, frames) for w in (1, 103, 129) for frames in (1, 5)]


@pytest.mark.parametrize("w,frames", OP_SHAPES)
def test_op_without_rescale_is_bit_equal(w, frames):
    """every (gain, scale) pair of {0, 1, 0.5, 2.5, -1} x {1, 1.25, 0, 2}, three clips at a time at their own timesteps, both table rows,
    ldo > w, the conditional half at Mc and at round_up(Mc, 256), with and without x0, eps at a column offset"""
    n = 0
    for sc, ts in S.pair_cases():
        for cond_pad in (False, True):
            for which, c0, x0_on in ((0, 0, True), (1, 3, False), (1, 0, True)):
                t = S.sched_inputs(w, frames, sc, ts, which=which, c0=c0, cond_pad=cond_pad, ld_extra=3 + 2 * which)
                e_ref, x0_ref, _ = S.cfg_mix_sched_ref(t)
                e, x0 = _op(t, x0_on)
                assert torch.equal(e, e_ref), (sc, ts, cond_pad, which)
                assert x0 is None or torch.equal(x0, x0_ref), (sc, ts, cond_pad, which)
                n += 1
    assert n == 42
    # the gain-1 shortcut at a scale for which 1 + (s - 1) is not s in fp32, and timesteps outside the table (clamped, never read outside)
    t = S.sched_inputs(w, frames, (0.15, 0.15, 2.0), (1, 1, 1))
    assert torch.equal(_op(t)[0], S.cfg_mix_sched_ref(t)[0])
    t = S.sched_inputs(w, frames, (2.0, 2.0, 2.0), (-5, 7, 1 << 40))
    assert torch.equal(_op(t)[0], S.cfg_mix_sched_ref(t)[0])
    # a table of ones is the plain mix, bit for bit
    t = S.sched_inputs(w, frames, (1.0, 1.15, 0.0), (0, 3, 6), table=torch.ones(2, 7))
    e, x0 = _op(t)
    e0, x00 = R.cfg_mix_ref(t)
    assert torch.equal(e, e0) and torch.equal(x0, x00)


@pytest.mark.parametrize("phi", [0.7, 1.0])
@pytest.mark.parametrize("w,frames", OP_SHAPES)
def test_op_with_rescale_within_two_ulp(w, frames, phi):
    """lens = [frames, 1, 3] (within the window), NaN in the padded frames of both halves of o: every valid element of eps within 2 fp32 ulp
    of the emulation, whose statistics are numpy's two-pass fp64; x0 exactly c1 x - c2 e' of the device's own e'"""
    lens = [frames, 1, min(3, frames)]
    worst = 0
    for sc, ts in S.pair_cases():
        for cond_pad, which, x0_on in ((False, 0, True), (True, 1, True), (True, 0, False)):
            t = S.sched_inputs(w, frames, sc, ts, which=which, phi=phi, lens=lens, cond_pad=cond_pad, ld_extra=3)
            e_ref, x0_ref, f = S.cfg_mix_sched_ref(t)
            e, x0 = _op(t, x0_on, nan_pad=True)
            v = S.valid_mask(t)
            assert bool(torch.isfinite(e[v]).all())
            de = int(S.ulp_distance(e[v], e_ref[v]).max())
            # x0 = c1 x - c2 e': an e' off by d ulp moves the subtraction's result by up to d ulp OF THE PRODUCT c2 e', which can be many ulp of
            # a cancelled difference — so x0 is held against the emulation's own arithmetic on the device's e'
            worst = max(worst, de)
            assert de <= ULPS, (sc, ts, which, de, f)
            if x0_on:
                b = torch.arange(t["Mc"]) // frames
                x0_dev = t["c1"][b][:, None] * t["x"][:, t["c0"]:t["c0"] + w] - t["c2"][b][:, None] * e
                assert torch.equal(x0[v], x0_dev[v]), (sc, ts, which)
    print(f"[cfg_mix_sched rescale w {w} frames {frames} phi {phi}] worst valid element: {worst} ulp from the emulation (gate {ULPS})")


@pytest.mark.parametrize("frames,lens", [(19, [19, 9, 3]), (16, [16, 8, 1]), (140, [140, 129, 7])])
def test_op_rescale_over_several_row_chunks(frames, lens):
    """the second launch walks a clip in chunks of 8 rows and a thread sums the moments of rows i, i + 128, ...: windows of more than one chunk,
    with a partial last one, and of more than 128 rows"""
    for w, phi in ((129, 0.7), (103, 1.0)):
        t = S.sched_inputs(w, frames, (2.0, 1.25, 2.0), (2, 3, 4), phi=phi, lens=lens)
        e_ref, _, f = S.cfg_mix_sched_ref(t)
        e, x0 = _op(t, nan_pad=True)
        v = S.valid_mask(t)
        assert all(x != 1 for x in f) and bool(torch.isfinite(e[v]).all())
        assert int(S.ulp_distance(e[v], e_ref[v]).max()) <= ULPS
        b = torch.arange(t["Mc"]) // frames
        assert torch.equal(x0[v], (t["c1"][b][:, None] * t["x"][:, :w] - t["c2"][b][:, None] * e)[v])


def test_op_rescale_exact_cases():
    # n = 1: one frame of one column — f = 1, the un-rescaled mix
    t = S.sched_inputs(1, 1, (2.0, 2.0, 2.0), (1, 1, 1), phi=1.0)
    e, x0 = _op(t)
    e_ref, x0_ref, f = S.cfg_mix_sched_ref(t)
    assert bool((f == 1).all()) and torch.equal(e, e_ref) and torch.equal(x0, x0_ref)
    assert torch.equal(e, S.cfg_mix_sched_ref(dict(t, phi=0.0))[0])
    # a clip of constant e: sigma_e = 0 exactly, f = 1
    for w in (103, 129):
        t = S.sched_inputs(w, 5, (2.0, 2.0, 2.0), (1, 1, 1), phi=0.7)
        t["o"][0:5] = 0.1
        t["o"][t["cond_row0"]:t["cond_row0"] + 5] = 0.7
        e, x0 = _op(t)
        e_ref, x0_ref, f = S.cfg_mix_sched_ref(t)
        assert f[0] == 1 and f[1] != 1
        assert torch.equal(e[:5], e_ref[:5]) and torch.equal(x0[:5], x0_ref[:5]) and len(set(e[:5].reshape(-1).tolist())) == 1
    # s_eff = 1 (gain 0 at scale 2, and scale 1 at any gain): the conditional prediction itself, whatever phi
    t = S.sched_inputs(129, 5, (2.0, 1.0, 2.0), (0, 3, 1), phi=1.0)
    e, _ = _op(t)
    k = t["o"][t["cond_row0"]:t["cond_row0"] + 15, :129]
    assert torch.equal(e[:10], k[:10]) and not torch.equal(e[10:], k[10:])


@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_op_rows_do_not_depend_on_the_batch(phi):
    """clip 1 of one batch as clip 0 of another (other neighbours, other scales and timesteps around it): the same bits"""
    for w, frames in ((103, 5), (129, 5), (1, 1)):
        lens = [frames, min(3, frames), 1] if phi else None
        a = S.sched_inputs(w, frames, (2.0, 1.25, 0.0), (2, 3, 4), phi=phi, lens=lens)
        b = S.sched_inputs(w, frames, (1.25, 2.0, 1.0), (3, 0, 1), phi=phi, lens=None if lens is None else [lens[1], lens[0], lens[2]], seed=5)
        F_ = frames
        b["o"][0:F_] = a["o"][F_:2 * F_]                                                       # u of clip 1 -> clip 0
        b["o"][b["cond_row0"]:b["cond_row0"] + F_] = a["o"][a["cond_row0"] + F_:a["cond_row0"] + 2 * F_]
        b["x"][0:F_] = a["x"][F_:2 * F_]
        b["c1"][0], b["c2"][0] = a["c1"][1], a["c2"][1]
        ea, xa = _op(a)
        eb, xb = _op(b)
        n = F_ if lens is None else lens[1]
        assert torch.equal(ea[F_:F_ + n], eb[:n]) and torch.equal(xa[F_:F_ + n], xb[:n]), (w, frames)


def test_op_undoubled_batch_is_the_plain_copy_and_bad_arguments():
    t = S.sched_inputs(103, 5, (2.0, 2.0, 2.0), (1, 1, 1))
    d = {n: t[n].to(DEV) for n in ("o", "x", "c1", "c2")}
    eps = torch.zeros(t["Mc"], t["lde"], device=DEV)
    lib = _lib.lib()
    # has_null = 0: the schedule is inert (no scales, timesteps or table needed)
    _lib.check(lib.dsh_op_cfg_mix_sched(None, _p(d["o"]), t["ldo"], t["Mc"], 0, 5, 103, 0, None, 0, _p(eps), t["lde"], 0, None, 0, None, None, None, 0,
                                        None, 0, None, 0, 0, 0.0, None))
    torch.cuda.synchronize()
    assert torch.equal(eps.cpu()[:, :103], t["o"][:t["Mc"], :103])
    tab, tt, sc = t["table"].to(DEV), t["t"].to(DEV), t["scale"].to(DEV)
    call = lambda phi, which, table: lib.dsh_op_cfg_mix_sched(None, _p(d["o"]), t["ldo"], t["Mc"], t["cond_row0"], 5, 103, 1, _p(sc), 1, _p(eps), t["lde"], 0,
                                                              None, 0, None, None, None, 0, _p(tt), 1, table, 7, which, phi, None)
    assert call(1.5, 0, _p(tab)) == -1 and call(-0.1, 0, _p(tab)) == -1 and call(0.5, 2, _p(tab)) == -1 and call(0.5, 0, None) == -1
    assert call(0.5, 1, _p(tab)) == 0


# =========================================================== model level ===========================================================
_MODELS = {}


def _model(precision="fp32", ds="show", single=False):
    key = (ds, precision, single)
    if key not in _MODELS:
        cfg = get_config(ds, unidiffuser=not single)
        cls = MotionTransformer if single else UniDiffuser
        sd = make_synthetic_state_dict(cfg, 1234) if single else synthetic_sd(ds)
        _MODELS[key] = cls(cfg, sd, device=DEV, precision=precision)
    m = _MODELS[key]
    m.set_guidance_scale(None)
    m.set_guidance_schedule(None)
    return m


def _eval(model, inp, t=560, c1=4.9, c2=4.8, lengths=None):
    cfg = model.cfg
    B, T = inp["x_T"].shape[:2]
    shape_e = (B, T, cfg.expression_dim)
    tt = t if torch.is_tensor(t) else torch.full((B,), int(t), dtype=torch.long)
    c1t = c1 if torch.is_tensor(c1) else torch.full((B,), float(c1))
    c2t = c2 if torch.is_tensor(c2) else torch.full((B,), float(c2))
    return model(inp["x_T"].cuda(), tt.cuda(), sqrt_alphas=[c1t.view(B, 1, 1).expand(shape_e), c2t.view(B, 1, 1).expand(shape_e)],
                 audio_emb=inp["audio_emb"].cuda(), length=None if lengths is None else torch.tensor(lengths), person_id=inp["person_id"].cuda(),
                 add_cond={"pretrain_aud_feat": inp["pretrain_aud_feat"].cuda()}, pe_type="pe_sinu", y={}).cpu()


def _kwargs(inp, lengths=None):
    return {"audio_emb": inp["audio_emb"], "length": None if lengths is None else torch.tensor(lengths), "person_id": inp["person_id"],
            "add_cond": {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "y": {}, "pe_type": "pe_sinu"}


def _ddim(model, inp, lengths=None, **kw):
    cfg = model.cfg
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B, T = inp["x_T"].shape[:2]
    kw.setdefault("seed", 4321)
    out = tr.diffusion_ddim_val.ddim_sample_loop(model, (B, T, cfg.net_dim_pose), clip_denoised=False, model_kwargs=_kwargs(inp, lengths), **kw)
    return (out[0].cpu(), out[1].cpu()) if isinstance(out, tuple) else out.cpu()


def _flags():
    torch.cuda.synchronize()
    got = _lib.launch_counts()
    return got["sample_graph"], got["sample_pipe"], got["sample_streams"]


def _oracle(cfg, inp, t, c1, c2, scales, sched, lengths=None):
    """The scheduled evaluation composed on the CPU from oracle.denoiser_ref, clip by clip (a clip of a ragged batch is the clip alone at its
    length): per encoder u from cond_scale = 0 and k from cond_scale = 1, mixed at s_eff = 1 + gain[t_b] (s_b - 1), rescaled with fp64
    statistics over the clip's frames and the encoder's columns; the gesture encoder is fed the composed expression x0.  [B, T, C], padded
    frames 0."""
    sd = synthetic_sd("show")
    B, T = inp["x_T"].shape[:2]
    out = torch.zeros(B, T, cfg.net_dim_pose)
    cfg_u, cfg_k = dataclasses.replace(cfg, cond_scale=0.0), dataclasses.replace(cfg, cond_scale=1.0)
    for b in range(B):
        n = T if lengths is None else lengths[b]
        x, a, h, pid = inp["x_T"][b:b + 1, :n], inp["audio_emb"][b:b + 1, :n], inp["pretrain_aud_feat"][b:b + 1, :n], inp["person_id"][b:b + 1]
        tb, c1b, c2b = t[b:b + 1], float(c1[b]), float(c2[b])

        def mix(prefix, xin, expr, m):
            with torch.no_grad():
                u = denoiser_ref.motion_transformer(sd, prefix, cfg_u, xin, tb, audio256, pid, h, expr)
                k = denoiser_ref.motion_transformer(sd, prefix, cfg_k, xin, tb, audio256, pid, h, expr)
            g = float((sched.expression, sched.gesture)[m][int(tb)])
            s_eff = scales[b] if g == 1.0 else 1.0 + g * (scales[b] - 1.0)
            if s_eff == 1.0:
                return k
            e = u + s_eff * (k - u)
            phi = sched.rescale[m]
            if phi > 0 and e.numel() >= 2:
                sk, se = float(k.double().std()), float(e.double().std())        # (torch.std: unbiased)
                if np.isfinite(se) and se > 0:
                    e = e * (phi * sk / se + (1.0 - phi))
            return e
        with torch.no_grad():
            emb_a = denoiser_ref.mlp_embed(sd, "time_embed", denoiser_ref.timestep_embedding(tb, cfg.latent_dim))
            aud_feat = denoiser_ref.decoder_layer(sd, "encoder_aud", a, None, emb_a, cfg.num_heads, None, False)
        audio256 = torch.cat((a, aud_feat), dim=-1)
        ges_x, exp_x = x[..., :cfg.split_pos], x[..., cfg.split_pos:]
        eps_exp = mix("encoder_exp", exp_x, None, 0)
        eps_ges = mix("encoder_ges", ges_x, c1b * exp_x - c2b * eps_exp, 1)
        out[b, :n] = torch.cat((eps_ges, eps_exp), dim=-1)[0]
    return out


# ---- 1. the trivial schedule ---------------------------------------------------------------------------------------------------------
def test_trivial_schedule_and_clearing_give_the_unscheduled_bits():
    model = _model()
    inp = make_inputs(model.cfg, 2, seed=3)
    e0, x0 = _eval(model, inp), _ddim(model, inp)                       # (the config's scale 1.25: a doubled batch)
    model.set_guidance_schedule(CFGSchedule())                          # gains 1, phi 0: the scheduled launch, the same arithmetic
    assert model.guidance_schedule == CFGSchedule()
    assert torch.equal(_eval(model, inp), e0) and torch.equal(_ddim(model, inp), x0)
    model.set_guidance_schedule(CFGSchedule(0.5, 2.0, rescale=0.5))
    assert not torch.equal(_eval(model, inp), e0)
    model.set_guidance_schedule(None)
    assert model.guidance_schedule is None
    assert torch.equal(_eval(model, inp), e0) and torch.equal(_ddim(model, inp), x0)
    # an undoubled batch: the schedule is inert
    model.set_guidance_scale(1.0)
    e1 = _eval(model, inp)
    model.set_guidance_schedule(CFGSchedule(0.5, 2.0, rescale=0.5))
    assert torch.equal(_eval(model, inp), e1)
    model.set_guidance_schedule(None)
    model.set_guidance_scale(None)


# ---- 2. gain 0 -------------------------------------------------------------------------------------------------------------------------
def test_gain_zero_takes_the_conditional_prediction():
    """both batches are doubled (the third clip guides in both), so rows at s_eff = 1 and rows at scale 1 run the same launches"""
    model = _model()
    inp = make_inputs(model.cfg, 3, seed=4)
    zero = CFGSchedule(0.0, 0.0)
    model.set_guidance_scale([2.0, 1.15, 2.0])
    model.set_guidance_schedule(zero)
    e, x = _eval(model, inp), _ddim(model, inp)
    model.set_guidance_schedule(None)
    model.set_guidance_scale([1.0, 1.0, 2.0])
    e1, x1 = _eval(model, inp), _ddim(model, inp)
    model.set_guidance_scale(None)
    assert torch.equal(e[:2], e1[:2]) and torch.equal(x[:2], x1[:2])
    assert not torch.equal(e[2], e1[2])                                  # (the third clip: k under gain 0, guided at 2 without)


# ---- 3. per encoder --------------------------------------------------------------------------------------------------------------------
def test_gain_per_encoder():
    model = _model()
    cfg = model.cfg
    inp = make_inputs(cfg, 2, seed=5)
    sched = CFGSchedule(expression=0.5, gesture=1.0)                      # at scale 2: s_eff = 1.5 (expression), 2 (gesture), both exact
    model.set_guidance_scale(2.0)
    model.set_guidance_schedule(sched)
    e, x = _eval(model, inp), _ddim(model, inp)
    model.set_guidance_schedule(None)
    model.set_guidance_scale(1.5)
    e15, x15 = _eval(model, inp), _ddim(model, inp)
    model.set_guidance_scale(None)
    sp = cfg.split_pos
    assert torch.equal(e[..., sp:], e15[..., sp:]) and torch.equal(x[..., sp:], x15[..., sp:])       # the expression chain never reads the gestures
    assert not torch.equal(e[..., :sp], e15[..., :sp])
    ref = _oracle(cfg, inp, torch.full((2,), 560), [4.9, 4.9], [4.8, 4.8], [2.0, 2.0], sched)
    d = max_abs(e, ref)
    print(f"[cfg schedule per encoder fp32] max|eps - composed oracle| = {d:.3e}")
    assert d < FP32_ATOL
    # ... and the oracle's own uniform evaluation at 1.5 on the expression columns (the composition is the reference's mix)
    with torch.no_grad():
        uni = denoiser_ref.unidiffuser(synthetic_sd("show"), dataclasses.replace(cfg, cond_scale=1.5), inp["x_T"], torch.full((2,), 560), torch.tensor(4.9),
                                       torch.tensor(4.8), inp["audio_emb"], inp["person_id"], inp["pretrain_aud_feat"])
    assert max_abs(ref[..., sp:], uni[..., sp:]) < 1e-4


# ---- 4. per timestep -------------------------------------------------------------------------------------------------------------------
def test_gain_per_timestep_is_the_loop_restarted_at_the_other_scale():
    model = _model()
    cfg = model.cfg
    inp = make_inputs(cfg, 2, seed=6)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    tmap = tr.diffusion_ddim_val.timestep_map
    assert len(tmap) == 25
    sched = CFGSchedule.from_levels(tr.diffusion_ddim_val, [1.0] * 12 + [0.5] * 13)
    assert sched.expression[tmap[12]] == 0.5 and sched.expression[tmap[12] - 1] == 0.5 and sched.expression[tmap[11]] == 1.0
    assert sched == CFGSchedule(*(lambda t: 0.5 if t > tmap[11] else 1.0,) * 2)
    got = _ddim(model, inp, cond_scale=2.0, cfg_schedule=sched)
    assert model.guidance_schedule is None and model.guidance_scale is None       # (held for the call)
    # levels 24 .. 12 at 1.5, then levels 11 .. 0 at 2.0 from the traced state
    _, trace = _ddim(model, inp, cond_scale=1.5, return_trace=True)
    want = _ddim(model, inp, cond_scale=2.0, noise=trace[12].to(DEV), start_level=12)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert not torch.equal(got, _ddim(model, inp, cond_scale=2.0))


def test_gain_per_timestep_in_one_evaluation():
    model = _model()
    cfg = model.cfg
    inp = make_inputs(cfg, 2, seed=7)
    t = torch.tensor([560, 40])
    c1, c2 = torch.tensor([4.9, 1.2]), torch.tensor([4.8, 0.66])
    sched = CFGSchedule(expression=lambda k: 0.5 if k >= 300 else 2.5, gesture=lambda k: 0.0 if k >= 300 else -1.0)
    model.set_guidance_scale([2.0, 1.25])
    model.set_guidance_schedule(sched)
    e = _eval(model, inp, t, c1, c2)
    model.set_guidance_schedule(None)
    model.set_guidance_scale(None)
    ref = _oracle(cfg, inp, t, c1, c2, [2.0, 1.25], sched)
    d = max_abs(e, ref)
    print(f"[cfg schedule per timestep fp32] max|eps - composed oracle| = {d:.3e}")
    assert d < FP32_ATOL


# ---- 5. rescale ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
def test_rescale_against_the_composed_oracle(precision):
    model = _model(precision)
    cfg = model.cfg
    B = 6 if precision == "bf16x3" else 2                                 # (bf16x3: 528 token rows, above the 512-row limit of the split loop)
    lengths = [(88, 37)[b % 2] for b in range(B)]
    inp = make_inputs(cfg, B, seed=8)
    sched = CFGSchedule(rescale=(0.7, 0.3))
    model.set_guidance_scale(2.0)
    model.set_guidance_schedule(sched)
    _lib.launch_counts(reset=True)
    e = _eval(model, inp, 560, 4.9, 4.8, lengths)
    counts = _lib.launch_counts()
    plain = None
    if precision == "fp32":
        model.set_guidance_schedule(None)
        plain = _eval(model, inp, 560, 4.9, 4.8, lengths)
    model.set_guidance_schedule(None)
    model.set_guidance_scale(None)
    if precision == "bf16x3":
        assert_split_ran(counts, "rescale")
    ref = _oracle(cfg, inp, torch.full((B,), 560), [4.9] * B, [4.8] * B, [2.0] * B, sched, lengths)
    valid = torch.zeros(B, 88, dtype=torch.bool)
    for b, n in enumerate(lengths):
        valid[b, :n] = True
    d = (e - ref)[valid]
    dmax, rms = float(d.abs().max()), float(d.pow(2).mean().sqrt())
    print(f"[cfg schedule rescale {precision}] max|eps - composed oracle| = {dmax:.3e}, rms = {rms:.3e}")
    assert torch.isfinite(e[valid]).all()
    if precision == "bf16":
        assert dmax < BF16_MAX and rms < BF16_RMS
    else:
        assert dmax < FP32_ATOL
    if plain is not None:
        # the factor itself, on the expression columns (the gesture encoder also reads another expression x0): rescaled = f x un-rescaled,
        # one f per clip
        sp = cfg.split_pos
        for b, n in enumerate(lengths):
            r, p = e[b, :n, sp:].double(), plain[b, :n, sp:].double()
            f = float((r * p).sum() / (p * p).sum())
            print(f"[cfg schedule rescale fp32] clip {b} expression: f = {f:.6f}")
            assert f != 1.0 and 0.3 < f < 1.7 and float((r - f * p).abs().max()) < 1e-5 * float(p.abs().max()), (b, f)


def test_rescaled_ragged_loop_keeps_padded_frames_zero():
    model = _model()
    inp = make_inputs(model.cfg, 2, seed=9)
    sched = CFGSchedule(expression=0.75, rescale=(0.7, 0.3))
    x = _ddim(model, inp, lengths=[88, 37], cond_scale=2.0, cfg_schedule=sched, row_keys=[0, 1])
    assert torch.isfinite(x).all() and bool((x[1, 37:] == 0).all()) and float(x[1, :37].abs().max()) > 0
    # the short clip is the clip alone at its length
    one = {k: (v[1:2, :37] if v.dim() == 3 else v[1:2]) for k, v in inp.items()}
    alone = _ddim(model, one, cond_scale=2.0, cfg_schedule=sched, row_keys=[1])
    r = float((x[1, :37] - alone[0]).abs().max() / alone.abs().max())
    print(f"[cfg schedule ragged loop] short clip vs alone: {r:.3e} of the range")
    assert r < 1e-5                                                       # test_gpu_ragged's fp32 loop bar


# ---- 6. regimes ------------------------------------------------------------------------------------------------------------------------
SCHED_REGIME = dict(expression=lambda t: 0.5 if t >= 480 else 1.5, gesture=lambda t: 1.0 if t >= 200 else 0.0, rescale=(0.7, 0.3))


def test_every_loop_regime_equals_the_single_stream_eager_loop(monkeypatch):
    model = _model()
    inp = make_inputs(model.cfg, 2, seed=10)
    sched = CFGSchedule(**SCHED_REGIME)
    kw = dict(cond_scale=[2.0, 1.25], cfg_schedule=sched)
    monkeypatch.setenv("DSH_NO_GRAPH", "1")
    monkeypatch.setenv("DSH_PIPE", "0")
    _lib.launch_counts(reset=True)
    want = _ddim(model, inp, **kw)
    assert _flags() == (0, 0, 1) and torch.isfinite(want).all()
    monkeypatch.delenv("DSH_NO_GRAPH")
    monkeypatch.delenv("DSH_PIPE")
    for env, flags in (({}, (1, 1, 1)), ({"DSH_PIPE": "0"}, (1, 0, 1)), ({"DSH_NO_GRAPH": "1"}, (0, 1, 1))):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _lib.launch_counts(reset=True)
        got = _ddim(model, inp, **kw)
        f = _flags()
        for k in env:
            monkeypatch.delenv(k)
        assert f == flags, (env, f)
        assert torch.equal(got, want), (env, float((got - want).abs().max()))
    assert not torch.equal(want, _ddim(model, inp, cond_scale=[2.0, 1.25]))


def test_sub_batch_streams_equal_the_single_stream_eager_loop(monkeypatch):
    """B = 4 on two forced sub-batch streams (a context built under DSH_DUAL_MIN_ROWS / DSH_DUAL_ROWS, as test_gpu_editing does): every
    instance reads its own clips' timesteps, scales and lengths and the one schedule.  Each sub-batch equals the single-stream eager loop of
    its two clips (one Philox stream per clip: the same noise in either batch)."""
    cfg = get_config("show")
    inp = make_inputs(cfg, 4, seed=11)
    sched = CFGSchedule(**SCHED_REGIME)
    scales, lengths = [2.0, 1.25, 1.5, 2.0], [88, 37, 60, 88]
    monkeypatch.setenv("DSH_DUAL_MIN_ROWS", "64")
    monkeypatch.setenv("DSH_DUAL_ROWS", "128")
    monkeypatch.setenv("DSH_PIPE", "0")
    split = UniDiffuser(cfg, synthetic_sd("show"), device=DEV, precision="fp32")
    _lib.launch_counts(reset=True)
    got = _ddim(split, inp, lengths=lengths, cond_scale=scales, cfg_schedule=sched, row_keys=[0, 1, 2, 3])
    assert _flags() == (0, 0, 2)
    split.set_guidance_scale(scales)
    split.set_guidance_schedule(sched)
    e_split = _eval(split, inp, torch.tensor([560, 40, 560, 40]), 4.9, 4.8, lengths)
    split.close()
    monkeypatch.delenv("DSH_DUAL_MIN_ROWS")
    monkeypatch.delenv("DSH_DUAL_ROWS")
    monkeypatch.setenv("DSH_NO_GRAPH", "1")
    model = _model()
    for lo in (0, 2):
        part = {k: v[lo:lo + 2] for k, v in inp.items()}
        _lib.launch_counts(reset=True)
        want = _ddim(model, part, lengths=lengths[lo:lo + 2], cond_scale=scales[lo:lo + 2], cfg_schedule=sched, row_keys=[lo, lo + 1])
        assert _flags() == (0, 0, 1)
        assert torch.equal(got[lo:lo + 2], want), (lo, float((got[lo:lo + 2] - want).abs().max()))
        model.set_guidance_scale(scales[lo:lo + 2])
        model.set_guidance_schedule(sched)
        e = _eval(model, part, torch.tensor([560, 40]), 4.9, 4.8, lengths[lo:lo + 2])
        model.set_guidance_schedule(None)
        model.set_guidance_scale(None)
        for b in range(2):
            n = lengths[lo + b]
            assert torch.equal(e_split[lo + b, :n], e[b, :n]), (lo, b)


def test_one_modality_alone_reads_its_own_row():
    model = _model()
    cfg = model.cfg
    inp = make_inputs(cfg, 2, seed=12)
    sched = CFGSchedule(expression=0.5, gesture=2.5, rescale=(0.7, 0.3))
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    joint = tr.generate_batch(inp["audio_emb"], inp["person_id"], cfg.net_dim_pose, {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, {}, seed=3,
                              cond_scale=2.0, cfg_schedule=sched).cpu()
    face = tr.generate_batch(inp["audio_emb"], inp["person_id"], cfg.net_dim_pose, {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, {}, seed=3,
                             cond_scale=2.0, cfg_schedule=sched, modality="expression").cpu()
    sp = cfg.split_pos
    assert torch.equal(face[..., sp:], joint[..., sp:]) and bool((face[..., :sp] == 0).all())


# ---- the Python entry points -----------------------------------------------------------------------------------------------------------
def test_keyword_equals_the_sticky_setting_on_every_entry_point():
    model = _model()
    cfg = model.cfg
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    sched = CFGSchedule.interval(200, 799, rescale=0.5)
    N = cfg.n_poses + (cfg.n_poses - cfg.overlap_len)                     # two windows
    inp = make_inputs(cfg, 2, frames=N, seed=13)
    add = {"pretrain_aud_feat": inp["pretrain_aud_feat"]}
    win = {k: (v[:, :cfg.n_poses] if v.dim() == 3 else v) for k, v in inp.items()}
    wadd = {"pretrain_aud_feat": win["pretrain_aud_feat"]}
    motions = torch.randn(2, cfg.n_poses, cfg.net_dim_pose, generator=torch.Generator().manual_seed(3))
    x0 = torch.randn(2, cfg.n_poses, cfg.net_dim_pose, generator=torch.Generator().manual_seed(4)).to(DEV)
    calls = {
        "chain": lambda **kw: tr.sample_arbitrary_len(inp["audio_emb"], inp["person_id"], add, seed=7, row_keys=[0, 1], **kw),
        "ragged chain": lambda **kw: torch.cat(tr.sample_arbitrary_len(inp["audio_emb"], inp["person_id"], add, seed=7, row_keys=[0, 1],
                                                                       lengths=[N, 100], **kw), 0),
        "variations": lambda **kw: tr.sample_variations(motions, win["audio_emb"], win["person_id"], wadd, level=10, seed=5, **kw),
        "losses": lambda **kw: tr.diffusion_ddim_val.training_losses(model, x0, [3, 20], _kwargs(win), seed=9, **kw)["pred"],
    }
    for name, call in calls.items():
        base = call().clone()
        got = call(cfg_schedule=sched).clone()
        assert model.guidance_schedule is None, name
        model.set_guidance_schedule(sched)
        want = call().clone()
        model.set_guidance_schedule(None)
        assert torch.isfinite(got).all() and torch.equal(got, want) and not torch.equal(got, base), name


# ---- 7. argument rules -----------------------------------------------------------------------------------------------------------------
def _c_set(model, ge, gg, n, pe, pg):
    fp = C.POINTER(C.c_float)
    a = None if ge is None else np.ascontiguousarray(ge, dtype=np.float32)
    b = None if gg is None else np.ascontiguousarray(gg, dtype=np.float32)
    return _lib.lib().dsh_set_guidance_schedule(model._h, None if a is None else a.ctypes.data_as(fp), None if b is None else b.ctypes.data_as(fp), n,
                                                C.c_float(pe), C.c_float(pg))


def test_c_entry_refuses_before_any_state_changes():
    model = _model()
    inp = make_inputs(model.cfg, 2, frames=24, seed=14)
    sticky = CFGSchedule(0.5, 1.5, rescale=0.25)
    model.set_guidance_schedule(sticky)
    base = _eval(model, inp)
    ones, nan, inf = np.ones(1000), np.ones(1000), np.ones(1000)
    nan[17], inf[999] = float("nan"), float("inf")
    bad = [(nan, ones, 1000, 0, 0), (ones, inf, 1000, 0, 0), (ones, ones, 1000, 1.5, 0), (ones, ones, 1000, 0, -0.1), (ones, ones, 1000, float("nan"), 0),
           (ones, ones, 999, 0, 0), (ones, ones, 1001, 0, 0), (ones, ones, -1, 0, 0), (None, ones, 1000, 0, 0), (ones, None, 1000, 0, 0)]
    for args in bad:
        assert _c_set(model, *args) == -1, args[2:]
        assert _lib.lib().dsh_last_error()
        assert torch.equal(_eval(model, inp), base), args[2:]             # the sticky schedule still holds
    assert _c_set(model, None, None, 0, 0, 0) == 0                        # n_steps = 0 clears (the arrays are not read)
    model._schedule = None
    assert not torch.equal(_eval(model, inp), base)
    assert _c_set(model, sticky.expression, sticky.gesture, 1000, *sticky.rescale) == 0
    assert torch.equal(_eval(model, inp), base)
    model.set_guidance_schedule(None)
    # weights without classifier_free: only the trivial schedule
    beat = _model(ds="beat")
    half = np.full(1000, 0.5)
    assert _c_set(beat, half, ones, 1000, 0, 0) == -1 and _c_set(beat, ones, ones, 1000, 0, 0.5) == -1
    assert _c_set(beat, ones, ones, 1000, 0, 0) == 0 and _c_set(beat, None, None, 0, 0, 0) == 0
    # one encoder: the two rows and the two factors must be equal
    single = _model("bf16", single=True)
    assert _c_set(single, half, ones, 1000, 0, 0) == -1 and _c_set(single, half, half, 1000, 0.5, 0.25) == -1
    assert _c_set(single, half, half, 1000, 0.5, 0.5) == 0 and _c_set(single, None, None, 0, 0, 0) == 0


def test_python_refusals_and_the_sticky_setting_survives(monkeypatch):
    model = _model()
    cfg = model.cfg
    inp = make_inputs(cfg, 2, frames=24, seed=15)
    sticky = CFGSchedule(0.5, 1.5, rescale=0.25)
    model.set_guidance_schedule(sticky)
    base = _ddim(model, inp)
    for bad in (CFGSchedule(steps=500), "interval", 0.5):
        with pytest.raises(ValueError):
            model.set_guidance_schedule(bad)
        with pytest.raises(ValueError):
            _ddim(model, inp, cfg_schedule=bad)
    assert model.guidance_schedule == sticky
    # a cfg_schedule= call whose native loop fails: the sticky schedule comes back
    other = CFGSchedule.interval(100, 900)
    lib = _lib.lib()
    monkeypatch.setattr(lib, "dsh_sample_run", lambda *a: -1)
    with pytest.raises(_lib.DshError):
        _ddim(model, inp, cfg_schedule=other, cond_scale=2.0)
    monkeypatch.undo()
    assert model.guidance_schedule == sticky and model.guidance_scale is None
    assert torch.equal(_ddim(model, inp), base)
    # ... and one refused while it is being set (per-clip scales of the wrong length are refused before the schedule is touched)
    with pytest.raises(ValueError):
        _ddim(model, inp, cfg_schedule=other, cond_scale=[1.1, 1.2, 1.3])
    assert model.guidance_schedule == sticky and torch.equal(_ddim(model, inp), base)
    model.set_guidance_schedule(None)
    # BEAT: no classifier-free weights
    beat = _model(ds="beat")
    binp = make_inputs(beat.cfg, 2, seed=3)
    for bad in (CFGSchedule(0.5), CFGSchedule(rescale=0.5)):
        with pytest.raises(ValueError):
            beat.set_guidance_schedule(bad)
        with pytest.raises(ValueError):
            _ddim(beat, binp, cfg_schedule=bad)
    b0 = _ddim(beat, binp)
    assert torch.equal(_ddim(beat, binp, cfg_schedule=CFGSchedule()), b0)  # the trivial one is accepted and inert
    # the single transformer takes the rows only when they are equal
    single = _model("bf16", single=True)
    with pytest.raises(ValueError):
        single.set_guidance_schedule(CFGSchedule(0.5, 1.0))
    with pytest.raises(ValueError):
        single.set_guidance_schedule(CFGSchedule(rescale=(0.5, 0.25)))
    sinp = make_inputs(single.cfg, 2, seed=3)
    tr = DDPMTrainer(sampler_namespace(single.cfg), single)
    run = lambda **kw: tr.diffusion_ddim_val.ddim_sample_loop(single, (2, single.cfg.n_poses, single.cfg.net_dim_pose), clip_denoised=False,
                                                              model_kwargs=_kwargs(sinp), seed=2, **kw).cpu()
    s0 = run()
    single.set_guidance_scale(1.125)                                       # 1 + 0.5 (1.25 - 1)
    s1 = run()
    single.set_guidance_scale(None)
    assert torch.equal(run(cfg_schedule=CFGSchedule(0.5, 0.5)), s1) and not torch.equal(s0, s1)
