"""Synchronised window batches end to end, on a real MI355X: every window of a long stream is one row of ONE batch, the
rows run the plain 25-step loop together and behind every step the frames two neighbouring windows share are reconciled.

BEAT synthetic weights (n_poses = 34, overlap_len = 4, C = 192), fp32 and bf16.  The main stream has 109 frames: windows of 34, 34, 34
and a 19-frame tail, 4 rows, a ragged batch.  SHOW is added where classifier-free guidance matters.

Gates.  Bit-identity wherever the project already has it (the two-encoder pipeline against one chain, one modality alone against the
joint run, a refused call leaving nothing behind).  Against a replay through the operator boundary and for a stream alone against the
same stream in a larger batch: the project's batch-vs-alone gates, 1e-5 of the result's range in fp32, 1.2e-2 in bf16 —
the operator boundary and the loop, or two batch sizes, may choose different launch regimes, which is what those gates cover.

The per-step property is checked on a traced run.  A trace switches the two-encoder pipeline off (sampler.hip, plan(): it needs all
channels of a step at once), so the pipelined regime is shown by its launch counter on an untraced run whose result must equal the
traced run's bit for bit, and whose shared frames are checked on the final windows."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsheg_amd import _lib, glue  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.glue import CFGSchedule, MotionGuidance  # noqa: E402
from diffsheg_amd.synthetic import SeededNoise, make_inputs, make_pose_stat_vectors  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace, stitch_synchronised, synchronised_window_plan  # noqa: E402
from synchronised_ref import copies_equal, max_copy_gap, window_sync  # noqa: E402
from test_gpu_dispatch_sweep import n_streams  # noqa: E402  (the sub-batch split rule, restated there)
from util import gpu_model, rel_err  # noqa: E402

DEV = "cuda:0"
GATE = {"fp32": 1e-5, "bf16": 1.2e-2}            # a clip of a batch against the clip alone (test_gpu_dispatch_sweep.LOOP_TOL)
N_MAIN = 109                                     # 34 + 30 + 30 + 15: three full windows and a 19-frame tail
PRECS = ["fp32", "bf16"]


def _trainer(prec, ds="beat", **over):
    cfg = get_config(ds)
    return cfg, gpu_model(ds, prec), DDPMTrainer(sampler_namespace(cfg, **over), gpu_model(ds, prec))


def _streams(cfg, S, N, seed=61):
    inp = make_inputs(cfg, S, frames=N, seed=seed)
    return inp["audio_emb"].to(DEV), inp["pretrain_aud_feat"].to(DEV), inp["person_id"].to(DEV)


def _cut(t, plan):
    """[S, N, ...] -> the plan's rows [rows, T, ...], zero behind every row's length (row by row: the test's own restatement)"""
    out = t.new_zeros((len(plan["stream"]), plan["frames"]) + tuple(t.shape[2:]))
    for r, (s, st, n) in enumerate(zip(plan["stream"], plan["start"], plan["lengths"])):
        out[r, :n] = t[s, st:st + n]
    return out


def _batch(cfg, tr, audio, hub, pid, seed, keys=None, lengths=None):
    """the window batch of the streams, as sample_arbitrary_len_synchronised builds it: (plan, model_kwargs, x_T)"""
    S, N = audio.shape[:2]
    plan = synchronised_window_plan(lengths or [N] * S, cfg.n_poses, cfg.overlap_len)
    z = tr.diffusion_ddim_val.draw_noise(S, N, cfg.net_dim_pose, DEV, seed, keys or list(range(S)), None, lengths)
    kw = {"audio_emb": _cut(audio, plan), "length": torch.tensor(plan["lengths"]), "person_id": pid[plan["stream"]],
          "add_cond": {"pretrain_aud_feat": _cut(hub, plan)}, "y": {}, "pe_type": "pe_sinu"}
    return plan, kw, _cut(z, plan)


def _fresh(kw):
    """new tensor objects: the context is conditioned again, under the switches of the moment"""
    return dict(kw, audio_emb=kw["audio_emb"].clone(), person_id=kw["person_id"].clone(),
                add_cond={"pretrain_aud_feat": kw["add_cond"]["pretrain_aud_feat"].clone()})


def _loop(tr, model, kw, xT, **more):
    return tr.diffusion_ddim_val.ddim_sample_loop(model, tuple(xT.shape), noise=xT, clip_denoised=False, model_kwargs=kw, seed=1, **more)


# ---- 1. every step is synchronised, in both regimes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_every_step_is_synchronised(prec, monkeypatch):
    cfg, model, tr = _trainer(prec)
    audio, hub, pid = _streams(cfg, 1, N_MAIN)
    plan, kw, xT = _batch(cfg, tr, audio, hub, pid, seed=5)
    left, lens, L = plan["left"], plan["lengths"], cfg.overlap_len
    assert lens == [34, 34, 34, 19] and left == [-1, 0, 1, 2] and plan["frames"] == 34
    assert copies_equal(xT, left, L, lens)                                    # ONE noise value per stream frame
    sync = dict(sync_left=left, sync_len=L)
    # the default regime: the two-encoder pipeline, each chain reconciling its own columns on its own stream
    _lib.launch_counts(reset=True)
    piped = _loop(tr, model, kw, xT, **sync).clone()
    torch.cuda.synchronize()
    got = _lib.launch_counts()
    assert got["sample_pipe"] == 1 and got["sample_streams"] == 1, got
    assert torch.isfinite(piped).all() and copies_equal(piped, left, L, lens)
    # traced (one chain): the two copies of every shared frame are bit-identical after every one of the 25 steps
    _lib.launch_counts(reset=True)
    x, trace = _loop(tr, model, kw, xT, return_trace=True, **sync)
    torch.cuda.synchronize()
    assert _lib.launch_counts()["sample_pipe"] == 0 and trace.shape[0] == 25
    for i in range(25):
        assert copies_equal(trace[i], left, L, lens), (i, max_copy_gap(trace[i], left, L, lens))
    valid = torch.arange(34, device=DEV)[None, :, None] < torch.tensor(lens, device=DEV)[:, None, None]
    assert torch.equal(x, torch.where(valid, trace[-1], torch.zeros_like(x)))      # (the last step, padded frames zeroed)
    # the pipeline switched off, untraced
    monkeypatch.setenv("DSH_PIPE", "0")
    _lib.launch_counts(reset=True)
    plain = _loop(tr, model, _fresh(kw), xT, **sync).clone()
    torch.cuda.synchronize()
    got = _lib.launch_counts()
    assert got["sample_pipe"] == 0 and got["sample_streams"] == 1, got
    # ... and all three are the same sample (the pipeline's existing property)
    assert torch.equal(piped, plain), float((piped - plain).abs().max())
    assert torch.equal(piped, x), float((piped - x).abs().max())


# ---- 2. the sync does something; without neighbours the call is what it was ----------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_without_neighbours_the_windows_part_and_the_loop_is_unchanged(prec):
    cfg, model, tr = _trainer(prec)
    audio, hub, pid = _streams(cfg, 1, N_MAIN)
    plan, kw, xT = _batch(cfg, tr, audio, hub, pid, seed=5)
    left, lens, L = plan["left"], plan["lengths"], cfg.overlap_len
    free = _loop(tr, model, kw, xT, sync_left=[-1] * 4, sync_len=L).clone()
    gap = max_copy_gap(free, left, L, lens)
    print(f"[{prec}] unsynchronised windows: largest gap between the two copies of a shared frame {gap:.3e} (range {float(free.abs().max()):.3e})")
    assert not copies_equal(free, left, L, lens) and gap > 0
    old = _loop(tr, model, kw, xT)
    assert torch.equal(free, old)
    synced = _loop(tr, model, kw, xT, sync_left=left, sync_len=L)
    assert copies_equal(synced, left, L, lens) and not torch.equal(synced, free)
    assert torch.isfinite(synced).all()


# ---- 3. a stream of one window is generate_batch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", [20, 34])
def test_single_window_equals_generate_batch(prec, N):
    cfg, model, tr = _trainer(prec)
    audio, hub, pid = _streams(cfg, 2, N, seed=62)
    out, windows, plan = tr.sample_arbitrary_len_synchronised(audio, pid, {"pretrain_aud_feat": hub}, seed=9, row_keys=[4, 8], return_windows=True)
    assert plan["left"] == [-1, -1] and plan["lengths"] == [N, N] and tuple(out.shape) == (2, N, cfg.net_dim_pose)
    xT = tr.diffusion_ddim_val.draw_noise(2, N, cfg.net_dim_pose, DEV, 9, [4, 8])
    want = tr.generate_batch(audio, pid, cfg.net_dim_pose, {"pretrain_aud_feat": hub}, {}, noise=xT, seed=9)
    assert torch.equal(out, want) and torch.equal(windows, want)


# ---- 4. replay through the operator boundary --------------------------------------------------------------------------------------------------
def _scalars(dd, k):
    """what Sampler::step_consts hands the step kernel at spaced level k (fp64 table -> fp32; the previous level's roots taken in fp32)"""
    c1, c2 = float(np.float32(dd.sqrt_recip_alphas_cumprod[k])), float(np.float32(dd.sqrt_recipm1_alphas_cumprod[k]))
    abp = np.float32(dd.alphas_cumprod_prev[k])
    return c1, c2, float(np.sqrt(abp)), float(np.sqrt(np.float32(1) - abp))


def _replay(cfg, model, dd, kw, xT, left, lens, L):
    """evaluate through dsh_eval, dsh_op_ddim_step, the torch reconciliation of synchronised_ref.py: 25 times"""
    B, T, Cc = xT.shape
    x = xT.clone()
    shape_e = (B, T, cfg.expression_dim)
    for k in range(dd.num_timesteps - 1, -1, -1):
        c1, c2, sab, s1m = _scalars(dd, k)
        eps = model(x, torch.full((B,), dd.timestep_map[k], dtype=torch.long, device=DEV), sqrt_alphas=[torch.full(shape_e, c1), torch.full(shape_e, c2)],
                    audio_emb=kw["audio_emb"], length=kw["length"], person_id=kw["person_id"], add_cond=kw["add_cond"], pe_type="pe_sinu", y={})
        _lib.check(_lib.lib().dsh_op_ddim_step(None, x.data_ptr(), eps.data_ptr(), None, None, None, B, T, Cc, c1, c2, sab, s1m, 0, 0, 0, 0, 0, 0),
                   "dsh_op_ddim_step")
        x = window_sync(x, left, L, lens)
    valid = torch.arange(T, device=DEV)[None, :, None] < torch.tensor(lens, device=DEV)[:, None, None]
    return torch.where(valid, x, torch.zeros_like(x))


@pytest.mark.parametrize("prec", PRECS)
def test_native_loop_against_a_replay_through_the_operator_boundary(prec):
    cfg, model, tr = _trainer(prec)
    audio, hub, pid = _streams(cfg, 1, N_MAIN)
    plan, kw, xT = _batch(cfg, tr, audio, hub, pid, seed=5)
    left, lens, L = plan["left"], plan["lengths"], cfg.overlap_len
    native = _loop(tr, model, kw, xT, sync_left=left, sync_len=L).clone()
    replay = _replay(cfg, model, tr.diffusion_ddim_val, kw, xT, left, lens, L)
    err = rel_err(native, replay)
    print(f"[{prec}] native synchronised loop vs replay (dsh_eval + dsh_op_ddim_step + torch sync): max err / range {err:.3e}, "
          f"bit-identical: {torch.equal(native, replay)}")
    assert copies_equal(replay, left, L, lens)
    assert err < GATE[prec], err
    if prec == "fp32":              # measured bit-identical at these shapes (4 rows: both sides run the few-row fp32 kernels): held to that
        assert torch.equal(native, replay)
    # the trainer's entry is this call: same plan, same x_T, same conditioning
    out, windows, p2 = tr.sample_arbitrary_len_synchronised(audio, pid, {"pretrain_aud_feat": hub}, seed=5, return_windows=True)
    assert p2 == plan and torch.equal(windows, native)
    assert torch.equal(out[0], stitch_synchronised(native, plan, L)[0]) and tuple(out.shape) == (1, N_MAIN, cfg.net_dim_pose)


# ---- 5. a stream alone and beside another stream ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_a_stream_does_not_depend_on_the_batch_around_it(prec):
    cfg, model, tr = _trainer(prec)
    audio, hub, pid = _streams(cfg, 2, N_MAIN, seed=63)
    cond = {"pretrain_aud_feat": hub}
    alone = tr.sample_arbitrary_len_synchronised(audio[:1], pid[:1], {"pretrain_aud_feat": hub[:1]}, seed=21, row_keys=[7])
    both, windows, plan = tr.sample_arbitrary_len_synchronised(audio, pid, cond, seed=21, row_keys=[7, 9], lengths=[N_MAIN, 71], return_windows=True)
    assert plan["ranges"] == [(0, 4), (4, 7)] and plan["lengths"] == [34, 34, 34, 19, 34, 34, 11] and plan["left"] == [-1, 0, 1, 2, -1, 4, 5]
    assert isinstance(both, list) and [tuple(o.shape) for o in both] == [(N_MAIN, 192), (71, 192)]
    assert copies_equal(windows, plan["left"], cfg.overlap_len, plan["lengths"])
    err = rel_err(both[0], alone[0])
    other = tr.sample_arbitrary_len_synchronised(audio[:1], pid[:1], {"pretrain_aud_feat": hub[:1]}, seed=22, row_keys=[7])
    far = rel_err(other[0], alone[0])
    print(f"[{prec}] a stream alone vs beside a 71-frame stream: max err / range {err:.3e}; another seed: {far:.3e}")
    assert err < GATE[prec], err
    assert far > 0.1, far


# ---- 6. a batch the context conditions as sub-batch streams runs as one chain ------------------------------------------------------------------
def test_split_batch_runs_as_one_chain(monkeypatch):
    """BEAT fp32 with the pipeline switched off: 121 windows are 4 114 token rows, above the 4 096 from which the context conditions two
    sub-batch streams (which the plain loop then runs free through all steps).  Neighbouring windows would sit in different streams:
    with sync the run is one chain, whose evaluations still fork and join the sub-batch instances."""
    monkeypatch.setenv("DSH_PIPE", "0")
    cfg, model, tr = _trainer("fp32")
    rows = 121
    N = 34 + (rows - 1) * 30
    assert n_streams("fp32", rows, 34) == 2 and n_streams("fp32", rows - 1, 34) == 1
    audio, hub, pid = _streams(cfg, 1, N, seed=64)
    plan, kw, xT = _batch(cfg, tr, audio, hub, pid, seed=3)
    left, lens, L = plan["left"], plan["lengths"], cfg.overlap_len
    assert len(left) == rows and lens == [34] * rows
    _lib.launch_counts(reset=True)
    free = _loop(tr, model, kw, xT).clone()
    torch.cuda.synchronize()
    assert _lib.launch_counts()["sample_streams"] == 2                       # the plain loop: two free-running sub-batch streams
    _lib.launch_counts(reset=True)
    out = _loop(tr, model, kw, xT, sync_left=left, sync_len=L).clone()
    torch.cuda.synchronize()
    got = _lib.launch_counts()
    assert got["sample_streams"] == 1 and got["eval_streams"] == 2 and got["sample_pipe"] == 0 and got["sample_graph"] == 0, got
    assert torch.isfinite(out).all() and copies_equal(out, left, L, lens)
    assert not copies_equal(free, left, L, lens)
    # the windows at the sub-batch boundary (rows 59 | 60) are reconciled like the others
    assert torch.equal(out[59, -L:], out[60, :L]) and not torch.equal(free[59, -L:], free[60, :L])


# ---- 7. feature combinations -----------------------------------------------------------------------------------------------------------------
def test_dpm2m_on_logsnr8():
    cfg, model, tr = _trainer("fp32")
    audio, hub, pid = _streams(cfg, 1, N_MAIN)
    try:
        tr.set_sampling(8, "logsnr", "dpm2m")
        plan, kw, xT = _batch(cfg, tr, audio, hub, pid, seed=5)
        left, lens, L = plan["left"], plan["lengths"], cfg.overlap_len
        x, trace = _loop(tr, model, kw, xT, sync_left=left, sync_len=L, return_trace=True)
        assert trace.shape[0] == 8 and torch.isfinite(x).all()
        for i in range(8):                                                   # first-order and second-order steps alike
            assert copies_equal(trace[i], left, L, lens), i
        out, windows, _ = tr.sample_arbitrary_len_synchronised(audio, pid, {"pretrain_aud_feat": hub}, seed=5, return_windows=True)
        assert torch.equal(windows, x)                                       # set_sampling applies to the trainer's entry
        first = _loop(tr, model, kw, xT, sync_left=left, sync_len=L, solver="ddim")
        assert copies_equal(first, left, L, lens) and not torch.equal(first, x)
    finally:
        tr.set_sampling()


def test_keyframe_inside_an_overlap_and_velocity_damping():
    cfg, model, tr = _trainer("fp32")
    Cc, L = cfg.net_dim_pose, cfg.overlap_len
    audio, hub, pid = _streams(cfg, 1, N_MAIN)
    cond = {"pretrain_aud_feat": hub}
    kf = 31                                                                  # stream frame 31: frame 31 of window 0 and frame 1 of window 1
    Y = torch.zeros(1, N_MAIN, Cc, device=DEV)
    W = torch.zeros(1, N_MAIN, Cc, device=DEV)
    Y[0, kf] = 1.5
    W[0, kf] = 0.05
    g = MotionGuidance(Y, W, vel=torch.full((Cc,), 0.002, device=DEV))
    plain = tr.sample_arbitrary_len_synchronised(audio, pid, cond, seed=5)
    out, windows, plan = tr.sample_arbitrary_len_synchronised(audio, pid, cond, seed=5, guidance=g, return_windows=True)
    assert copies_equal(windows, plan["left"], L, plan["lengths"]) and torch.isfinite(out).all()
    assert torch.equal(windows[0, 31], windows[1, 1]) and torch.equal(out[0, kf], windows[0, 31])
    d_plain, d_guided = float((plain[0, kf] - 1.5).abs().mean()), float((out[0, kf] - 1.5).abs().mean())
    print(f"[keyframe in an overlap] mean |x - target| at the keyframe: unguided {d_plain:.3f}, guided {d_guided:.3f}")
    # (synthetic weights: samples range over +-1e3 and a stiff attraction diverges, so "closer to the target" is no property of this model;
    #  what holds by construction: the guided launch moves the sample, both windows alike, and with every gradient exactly 0 — weight 0, no
    #  stencil — the guided launch plus reconciliation is the unguided one bit for bit)
    assert not torch.equal(out, plain)
    zero = tr.sample_arbitrary_len_synchronised(audio, pid, cond, seed=5, guidance=MotionGuidance(Y, torch.zeros_like(W)))
    assert torch.equal(zero, plain)
    # stream-long terms only
    with pytest.raises(ValueError, match="stream-long"):
        tr.sample_arbitrary_len_synchronised(audio, pid, cond, seed=5, guidance=MotionGuidance(Y[:, :34].contiguous(), W[:, :34].contiguous()))


def test_show_with_a_guidance_interval():
    cfg, model, tr = _trainer("fp32", "show")
    N = 88 + 78 + 30                                                         # windows of 88, 88 and 40 frames
    audio, hub, pid = _streams(cfg, 1, N, seed=65)
    cond = {"pretrain_aud_feat": hub}
    sched = CFGSchedule.interval(200, 800)
    out, windows, plan = tr.sample_arbitrary_len_synchronised(audio, pid, cond, seed=5, cfg_schedule=sched, return_windows=True)
    assert plan["lengths"] == [88, 88, 40] and tuple(out.shape) == (1, N, cfg.net_dim_pose)
    assert copies_equal(windows, plan["left"], cfg.overlap_len, plan["lengths"]) and torch.isfinite(out).all()
    always = tr.sample_arbitrary_len_synchronised(audio, pid, cond, seed=5)
    unguided = tr.sample_arbitrary_len_synchronised(audio, pid, cond, seed=5, cond_scale=1.0)
    assert not torch.equal(out, always) and not torch.equal(out, unguided) and model.guidance_schedule is None


@pytest.mark.parametrize("prec", PRECS)
def test_expression_alone_is_the_joint_run_s_expression(prec):
    cfg, model, tr = _trainer(prec)
    S, L = cfg.split_pos, cfg.overlap_len
    audio, hub, pid = _streams(cfg, 1, N_MAIN)
    cond = {"pretrain_aud_feat": hub}
    joint = tr.sample_arbitrary_len_synchronised(audio, pid, cond, seed=5)
    face, windows, plan = tr.sample_arbitrary_len_synchronised(audio, pid, cond, seed=5, modality="expression", return_windows=True)
    assert float(face[..., :S].abs().max()) == 0
    assert torch.equal(face[..., S:], joint[..., S:])
    assert copies_equal(windows, plan["left"], L, plan["lengths"])


def test_euler_result_is_the_converted_default_result():
    cfg, model, tr = _trainer("fp32")
    audio, hub, pid = _streams(cfg, 1, N_MAIN)
    cond = {"pretrain_aud_feat": hub}
    stats = glue.PoseStats(**make_pose_stat_vectors(cfg.split_pos // 3, 5), device=DEV)
    tr.set_pose_stats(stats)
    default = tr.sample_arbitrary_len_synchronised(audio, pid, cond, seed=5)
    euler = tr.sample_arbitrary_len_synchronised(audio, pid, cond, seed=5, pose_rep="euler")
    assert torch.equal(euler, glue.axis_angle_to_euler(default, stats, split_pos=cfg.split_pos)) and not torch.equal(euler, default)
    lst = tr.sample_arbitrary_len_synchronised(audio, pid, cond, seed=5, pose_rep="euler", lengths=[N_MAIN])
    assert isinstance(lst, list) and torch.equal(lst[0], euler[0])


@pytest.mark.parametrize("prec", PRECS)
def test_lengths_form_with_a_stream_of_one_short_window(prec):
    cfg, model, tr = _trainer(prec)
    audio, hub, pid = _streams(cfg, 2, N_MAIN, seed=66)
    out, windows, plan = tr.sample_arbitrary_len_synchronised(audio, pid, {"pretrain_aud_feat": hub}, seed=5, lengths=[N_MAIN, 3],
                                                              return_windows=True)
    assert plan["lengths"] == [34, 34, 34, 19, 3] and plan["left"] == [-1, 0, 1, 2, -1]          # (3 frames: shorter than the overlap itself)
    assert [tuple(o.shape) for o in out] == [(N_MAIN, 192), (3, 192)] and all(torch.isfinite(o).all() for o in out)
    assert copies_equal(windows, plan["left"], cfg.overlap_len, plan["lengths"])
    assert float(windows[4, 3:].abs().max()) == 0 and float(windows[3, 19:].abs().max()) == 0     # padded frames of the raw batch are 0
    solo = tr.sample_arbitrary_len_synchronised(audio[1:, :3].contiguous(), pid[1:], {"pretrain_aud_feat": hub[1:, :3].contiguous()}, seed=5, row_keys=[1])
    assert rel_err(out[1], solo[0]) < GATE[prec]


# ---- 8. refusals, each before the context changes ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was():
    cfg, model, tr = _trainer("fp32")
    Cc, L = cfg.net_dim_pose, cfg.overlap_len
    audio, hub, pid = _streams(cfg, 1, N_MAIN)
    cond = {"pretrain_aud_feat": hub}
    plan, kw, xT = _batch(cfg, tr, audio, hub, pid, seed=5)
    left = plan["left"]
    ca, ch, cp = _streams(cfg, 3, 34, seed=67)

    def clip():
        return tr.generate_batch(ca, cp, Cc, {"pretrain_aud_feat": ch}, {}, seed=44, row_keys=[1, 2, 3]).clone()
    before = clip()
    dd = tr.diffusion_ddim_val
    sync = dict(sync_left=left, sync_len=L)
    mask = torch.zeros(4, 34, Cc, dtype=torch.bool, device=DEV)
    mask[:, :L] = True
    y_masked = {"gt": torch.zeros(4, 34, Cc, device=DEV), "outpainting_mask": mask, "outpainting_mask_any": True}
    python_level = [
        (NotImplementedError, "DDIM loop", lambda: _trainer("fp32", ddim=False)[2].sample_arbitrary_len_synchronised(audio, pid, cond, seed=5)),
        (TypeError, "DDIM loops only", lambda: tr.diffusion.p_sample_loop(model, tuple(xT.shape), noise=xT, clip_denoised=False, model_kwargs=kw, seed=1, **sync)),
        (ValueError, "eta must be 0", lambda: _loop(tr, model, kw, xT, eta=0.5, **sync)),
        (NotImplementedError, "no mask", lambda: _loop(tr, model, dict(kw, y=y_masked), xT, **sync)),
        (NotImplementedError, "same_overlap_noisy", lambda: _trainer("fp32", same_overlap_noisy=True)[2].sample_arbitrary_len_synchronised(audio, pid, cond, seed=5)),
        (NotImplementedError, "same_overlap_noisy", lambda: _loop(_trainer("fp32", same_overlap_noisy=True)[2], model, kw, xT, **sync)),
        (NotImplementedError, "fix_very_first", lambda: _trainer("fp32", fix_very_first=True)[2].sample_arbitrary_len_synchronised(audio, pid, cond, seed=5)),
        (ValueError, "2 \\* overlap_len <= n_poses", lambda: _trainer("fp32", overlap_len=18)[2].sample_arbitrary_len_synchronised(audio, pid, cond, seed=5)),
        (ValueError, "overlap_len >= 1", lambda: _trainer("fp32", overlap_len=0)[2].sample_arbitrary_len_synchronised(audio, pid, cond, seed=5)),
        (NotImplementedError, "start_level", lambda: _loop(tr, model, kw, xT, start_level=5, **sync)),
        (NotImplementedError, "tail_blend", lambda: _loop(tr, model, kw, xT, tail_blend=True, **sync)),
        (ValueError, "noise_source", lambda: dd.ddim_sample_loop(model, tuple(xT.shape), noise=xT, clip_denoised=False, model_kwargs=kw, noise_source=SeededNoise(3), **sync)),
        (ValueError, "noise=", lambda: dd.ddim_sample_loop(model, tuple(xT.shape), clip_denoised=False, model_kwargs=kw, seed=1, **sync)),
        (ValueError, "go together", lambda: _loop(tr, model, kw, xT, sync_left=left)),
        (ValueError, "one entry per batch row", lambda: _loop(tr, model, kw, xT, sync_left=left[:3], sync_len=L)),
    ]
    for exc, frag, call in python_level:
        with pytest.raises(exc, match=frag):
            call()
        assert torch.equal(clip(), before), frag
    # the geometry is the library's to refuse (check_run, against the condition's lengths): through the loop ...
    for bad, frag in (([-1, 0, 0, 2], "two rows"), ([-1, 0, 1, 3], "own left neighbour"), ([-1, 0, 1, 9], "outside the batch")):
        with pytest.raises(_lib.DshError, match=frag):
            _loop(tr, model, kw, xT, sync_left=bad, sync_len=L)
        assert torch.equal(clip(), before), frag
    with pytest.raises(_lib.DshError, match="shorter than overlap_len"):      # the 19-frame tail cannot share 20 frames
        _loop(tr, model, kw, xT, sync_left=[-1, -1, -1, 2], sync_len=20)
    with pytest.raises(_lib.DshError, match="2 \\* overlap_len"):             # ... nor a full window 18 at each end
        _loop(tr, model, kw, xT, sync_left=left, sync_len=18)
    assert torch.equal(clip(), before)
    # ... and through the C interface, where every refusal of the spec is check_run's: nothing is launched, x keeps its bits
    before = clip()                                                           # (conditions the context: 3 clips of 34 frames)
    x = torch.full((3, 34, Cc), 5.0, device=DEV)
    lib = _lib.lib()
    ok = dict(init=1, x=x.data_ptr(), sync_left=[-1, 0, 1], sync_len=L)
    gt = torch.zeros(3, 34, Cc, device=DEV)
    m8 = torch.ones(3, 34, Cc, dtype=torch.uint8, device=DEV)
    cases = [
        (dict(kind=1), ok, b"DDIM loops only"),
        (dict(eta=0.5), ok, b"eta must be 0"),
        (dict(), dict(ok, masked=1, gt=gt.data_ptr(), mask=m8.data_ptr()), b"no mask"),
        (dict(son=1), ok, b"same_overlap_noisy"),
        (dict(), dict(ok, tail_blend=1), b"tail blend"),
        (dict(), dict(ok, start_level=5), b"start level"),
        (dict(), dict(ok, invert_to=3), b"reverse loop"),
        (dict(noise_mode=0), ok, b"noise stack"),
        (dict(), dict(ok, init=0), b"init = 1"),
        (dict(), dict(ok, init=2), b"init = 1"),
        (dict(), dict(ok, sync_len=0), b"sync_len >= 1"),
        (dict(), dict(ok, sync_left=[-1, 0]), b"different batch size"),
        (dict(), dict(ok, sync_left=[-1, 0, 1, 2]), b"different batch size"),
        (dict(), dict(ok, sync_left=[1, 0, 1]), b"two rows"),
        (dict(), dict(ok, sync_len=18), b"2 * overlap_len"),
        (dict(), dict(ok, sync_len=35), b"shorter than overlap_len"),
    ]
    for ofields, sfields, frag in cases:
        o = dd._opts(ofields.get("kind", 0), False, ofields.get("noise_mode", 1), 3, 0, ofields.get("eta", 0.0))
        o.same_overlap_noisy = ofields.get("son", 0)
        spec = _lib.run_spec(**sfields)
        cur = model._enter()
        try:
            rc = lib.dsh_sample_run(model._h, C.byref(o), C.byref(spec))
        finally:
            model._exit(cur)
        assert rc == -1 and frag in lib.dsh_last_error(), (ofields, frag, lib.dsh_last_error())
        # the counting entry refuses what needs no context with the same words
        if frag not in (b"different batch size", b"two rows", b"2 * overlap_len", b"shorter than overlap_len"):
            assert lib.dsh_sample_count(C.byref(o), C.byref(spec), None, None) == -1 and frag in lib.dsh_last_error(), frag
    torch.cuda.synchronize()
    assert float((x - 5.0).abs().max()) == 0
    assert torch.equal(clip(), before)
    # the accepted spec runs on the same condition
    spec = _lib.run_spec(**ok)
    o = dd._opts(0, False, 1, 3)
    cur = model._enter()
    try:
        assert lib.dsh_sample_run(model._h, C.byref(o), C.byref(spec)) == 0, lib.dsh_last_error()
    finally:
        model._exit(cur)
    torch.cuda.synchronize()
    assert torch.isfinite(x).all() and copies_equal(x, [-1, 0, 1], L) and float((x - 5.0).abs().max()) > 0
    assert torch.equal(clip(), before)
