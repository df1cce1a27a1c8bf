"""The BEAT Euler tail on a real MI355X: the two rotation kernels against the reference's float64 results (tests/golden/rotations_beat.npz,
made by tests/golden/make_golden_rotations.py), their ragged and geometry rules bit for bit, and the trainer keyword ``pose_rep``.

Tolerances: no number is fixed here.  Every gate is MARGIN x eps_ref, eps_ref being the largest error of the reference's OWN float32 run
against its float64 run, over the same joints in the same quantity, computed from the fixture's arrays.  MARGIN = 4: the device's
sinf / cosf / atan2f / asinf are accurate to a few ulp where the host's libm is within one.  Angles are compared modulo 360 degrees.
"As matrices": the rotation matrix is rebuilt in float64 from the kernel's output and compared entry by entry with the matrix of the
float64 truth.  Two joints of the edge block lie EXACTLY on gimbal lock; there cos Y is rounding noise in any fp32 run, the reference's
included (its float32 and float64 runs differ by 0.5 as matrices on one of them, ``edge_exact_gimbal_ref_mat_err``), and only Y is
determined: they are checked for finiteness, |Y| <= 90 and sin Y (the matrix entry R02), not as whole matrices.

Reference: trainers/ddpm_beat_trainer.py:1044-1060, datasets/beat.py:376-401, datasets/rotation_converter.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rotation_ref as rr  # noqa: E402
from diffsheg_amd import glue  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.synthetic import make_inputs, make_pose_stat_vectors, make_rotation_edge_cases, make_rotation_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from util import golden, gpu_model  # noqa: E402

MARGIN = 4.0
DEV = "cuda:0"
_CACHE = {}


def _fx():
    """Fixture, regenerated inputs and statistics, and the yardsticks eps_ref - computed once, shared, never modified."""
    if not _CACHE:
        f = golden("rotations_beat.npz")
        B, T, J = int(f["batch"]), int(f["frames"]), int(f["joints"])
        st = make_pose_stat_vectors(J, int(f["stats_seed"]))
        x_aa, x_eu = make_rotation_inputs(B, T, J, int(f["input_seed"]))
        edge = make_rotation_edge_cases()
        n_f, n_i = edge["axis_angle"].shape[-1], edge["euler"].shape[-1]
        unit = lambda n: glue.PoseStats(torch.zeros(n), torch.ones(n), torch.zeros(n), torch.ones(n), device=DEV)  # noqa: E731
        st64 = {k: v.double().numpy() for k, v in st.items()}
        wc, se = f["well_conditioned"], f["settled"]
        e_wc, e_se = f["edge_fwd_well_conditioned"], f["edge_inv_settled"]
        gim, exact = f["edge_fwd_gimbal"], f["edge_fwd_exact_gimbal"]
        plain = ~(gim | exact)
        eps = {
            "fwd_mat": _mat_err_euler(f["euler_deg_f32"], f["euler_deg_f64"]).max(),
            "fwd_deg": np.abs(rr.wrap360(rr.joints(f["euler_deg_f32"]) - rr.joints(f["euler_deg_f64"])))[wc].max(),
            "fwd_std": _std_err(f["euler_std_f32"], f["euler_deg_f64"], st64)[wc].max(),
            "inv_mat": _mat_err_aa(_destd_aa(f["aa_std_f32"], st64), f["aa_f64"]).max(),
            "inv_vec": np.abs(rr.joints(_destd_aa(f["aa_std_f32"], st64)) - rr.joints(f["aa_f64"]))[se].max(),
            "edge_fwd_deg": np.abs(rr.wrap360(rr.joints(f["edge_euler_deg_f32"]) - rr.joints(f["edge_euler_deg_f64"])))[e_wc].max(),
            "edge_fwd_mat": _mat_err_euler(f["edge_euler_deg_f32"], f["edge_euler_deg_f64"])[0, 0][plain].max(),
            "edge_fwd_mat_gimbal": _mat_err_euler(f["edge_euler_deg_f32"], f["edge_euler_deg_f64"])[0, 0][gim].max(),
            "edge_inv_mat": _mat_err_aa(f["edge_aa_f32"], f["edge_aa_f64"]).max(),
            "edge_inv_vec": np.abs(rr.joints(f["edge_aa_f32"]) - rr.joints(f["edge_aa_f64"]))[e_se].max(),
        }
        assert all(np.isfinite(v) and v > 0 for v in eps.values()), eps
        _CACHE.update(f=f, B=B, T=T, J=J, st=st, st64=st64, stats=glue.PoseStats(**st, device=DEV), x_aa=x_aa, x_eu=x_eu, edge=edge,
                      unit_f=unit(n_f), unit_i=unit(n_i), eps={k: float(v) for k, v in eps.items()})
    return _CACHE


def _mat_err_euler(a, b):
    return np.abs(rr.euler_deg_to_matrix(rr.joints(a)) - rr.euler_deg_to_matrix(rr.joints(b))).max(axis=(-1, -2))


def _mat_err_aa(a, b):
    return np.abs(rr.axis_angle_to_matrix(rr.joints(a)) - rr.axis_angle_to_matrix(rr.joints(b))).max(axis=(-1, -2))


def _destd_aa(x_std, st64):
    return np.asarray(x_std, np.float64) * st64["std_axis_angle"] + st64["mean_axis_angle"]


def _destd_eu(x_std, st64):
    return np.asarray(x_std, np.float64) * st64["std_euler"] + st64["mean_euler"]


def _std_err(std_out, deg_f64, st64):
    """Error of a standardised Euler result against the float64 truth, in standardised units, the angle difference taken modulo 360."""
    d = rr.wrap360(_destd_eu(std_out, st64) - deg_f64)
    return np.abs(rr.joints(d / st64["std_euler"]))


def _gate(what, got, eps_name):
    c = _fx()
    gate = MARGIN * c["eps"][eps_name]
    print(f"[rotation] {what}: measured {float(got):.3e}, gate {gate:.3e} (= {MARGIN:g} x eps_ref[{eps_name}] {c['eps'][eps_name]:.3e})")
    assert float(got) <= gate, (what, float(got), gate)


def _np(t):
    return t.detach().cpu().numpy()


# ---- 1. forward, random block ---------------------------------------------------------------------------------------------------
def test_forward_random_block_in_place_from_the_wide_tensor():
    c = _fx()
    f, B, T, J = c["f"], c["B"], c["T"], c["J"]
    cfg = get_config("beat")
    assert (3 * J, cfg.net_dim_pose) == (cfg.split_pos, 192)
    expr = torch.randn(B, T, cfg.expression_dim, generator=torch.Generator().manual_seed(9))
    wide = torch.cat([c["x_aa"], expr], -1).to(DEV)
    out_std = glue.axis_angle_to_euler(wide, c["stats"], split_pos=cfg.split_pos)
    out_deg = glue.axis_angle_to_euler(wide, c["stats"], split_pos=cfg.split_pos, degrees=True)
    assert out_std.shape == out_deg.shape == wide.shape and out_std.data_ptr() != wide.data_ptr()
    assert torch.isfinite(out_std).all() and torch.isfinite(out_deg).all()
    assert torch.equal(out_std[..., cfg.split_pos:], wide[..., cfg.split_pos:]) and torch.equal(out_deg[..., cfg.split_pos:], wide[..., cfg.split_pos:])
    assert torch.equal(wide[..., :cfg.split_pos].cpu(), c["x_aa"])                       # the input is left alone
    deg, std = _np(out_deg[..., :cfg.split_pos]), _np(out_std[..., :cfg.split_pos])
    wc = f["well_conditioned"]
    _gate("forward random, as matrices (every joint)", _mat_err_euler(deg, f["euler_deg_f64"]).max(), "fwd_mat")
    _gate("forward random, angles in degrees (well conditioned)", np.abs(rr.wrap360(rr.joints(deg) - rr.joints(f["euler_deg_f64"])))[wc].max(), "fwd_deg")
    _gate("forward random, standardised output (well conditioned)", _std_err(std, f["euler_deg_f64"], c["st64"])[wc].max(), "fwd_std")
    # the two outputs are one computation: standardised = (degrees - mean) / std, two correctly rounded fp32 operations
    m, s = c["stats"].mean_euler, c["stats"].std_euler
    assert torch.equal(out_std[..., :cfg.split_pos], (out_deg[..., :cfg.split_pos] - m) / s)
    # the narrow tensor gives the same bits as the gesture columns read in place
    assert torch.equal(glue.axis_angle_to_euler(c["x_aa"].to(DEV), c["stats"]), out_std[..., :cfg.split_pos])


# ---- 2. forward, edge block ---------------------------------------------------------------------------------------------------------
def test_forward_edge_block():
    c = _fx()
    f = c["f"]
    out = glue.axis_angle_to_euler(c["edge"]["axis_angle"].to(DEV), c["unit_f"], degrees=True)
    std = glue.axis_angle_to_euler(c["edge"]["axis_angle"].to(DEV), c["unit_f"])
    assert torch.isfinite(out).all() and torch.equal(out, std)                           # mean 0 / std 1
    deg = rr.joints(_np(out))[0, 0]
    truth = rr.joints(f["edge_euler_deg_f64"])[0, 0]
    gim, exact, zero, wc = f["edge_fwd_gimbal"], f["edge_fwd_exact_gimbal"], f["edge_fwd_zero"], f["edge_fwd_well_conditioned"][0, 0]
    assert (deg[zero] == 0.0).all()                                                      # exact zeros in -> exact zeros out
    err_deg = np.abs(rr.wrap360(deg - truth)).max(-1)
    print("[rotation] forward edge, angle error per joint (deg):", np.array2string(err_deg, precision=3))
    _gate("forward edge, either side of the small-angle threshold", err_deg[1:3].max(), "edge_fwd_deg")
    _gate("forward edge, angles (well conditioned)", err_deg[wc].max(), "edge_fwd_deg")
    err_mat = np.abs(rr.euler_deg_to_matrix(deg) - rr.euler_deg_to_matrix(truth)).max(axis=(-1, -2))
    print("[rotation] forward edge, matrix error per joint:", np.array2string(err_mat, precision=3))
    _gate("forward edge, as matrices (angles to 2 pi - 0.1)", err_mat[~(gim | exact)].max(), "edge_fwd_mat")
    _gate("forward edge, as matrices (within 0.5 degrees of gimbal lock)", err_mat[gim].max(), "edge_fwd_mat_gimbal")
    assert (np.abs(deg[gim | exact, 1]) <= 90.0).all()
    _gate("forward edge, sin Y exactly at gimbal lock", np.abs(np.sin(np.radians(deg[exact, 1])) - np.sin(np.radians(truth[exact, 1]))).max(),
          "edge_fwd_mat")


# ---- 3. inverse -----------------------------------------------------------------------------------------------------------------------
def test_inverse_random_and_edge_blocks():
    c = _fx()
    f = c["f"]
    out = glue.euler_to_axis_angle(c["x_eu"].to(DEV), c["stats"])
    assert torch.isfinite(out).all()
    aa = _destd_aa(_np(out), c["st64"])
    _gate("inverse random, as matrices (every joint)", _mat_err_aa(aa, f["aa_f64"]).max(), "inv_mat")
    _gate("inverse random, vectors (settled)", np.abs(rr.joints(aa) - rr.joints(f["aa_f64"]))[f["settled"]].max(), "inv_vec")
    # the truth is the rotation of the Euler input itself
    _gate("inverse random, as matrices against the input", np.abs(rr.axis_angle_to_matrix(rr.joints(aa)) - rr.euler_deg_to_matrix(
        rr.joints(_destd_eu(c["x_eu"].numpy(), c["st64"])))).max(), "inv_mat")
    e = glue.euler_to_axis_angle(c["edge"]["euler"].to(DEV), c["unit_i"])
    assert torch.isfinite(e).all()
    e_aa = _np(e).astype(np.float64)
    err_mat = _mat_err_aa(e_aa, f["edge_aa_f64"])[0, 0]
    print("[rotation] inverse edge, matrix error per joint:", np.array2string(err_mat, precision=3))
    _gate("inverse edge, as matrices (every joint)", err_mat.max(), "edge_inv_mat")
    _gate("inverse edge, vectors (settled)", np.abs(rr.joints(e_aa) - rr.joints(f["edge_aa_f64"]))[f["edge_inv_settled"]].max(), "edge_inv_vec")
    assert (rr.joints(e_aa)[0, 0, 0] == 0.0).all()                                       # zero angles in -> the zero vector


# ---- 4. round trip on the device --------------------------------------------------------------------------------------------------------
def test_round_trips_on_the_device():
    c = _fx()
    both = c["eps"]["fwd_mat"] + c["eps"]["inv_mat"]
    x = c["x_aa"].to(DEV)
    back = glue.euler_to_axis_angle(glue.axis_angle_to_euler(x, c["stats"]), c["stats"])
    e1 = _mat_err_aa(_destd_aa(_np(back), c["st64"]), _destd_aa(c["x_aa"].numpy(), c["st64"])).max()
    y = c["x_eu"].to(DEV)
    back2 = glue.axis_angle_to_euler(glue.euler_to_axis_angle(y, c["stats"]), c["stats"])
    e2 = _mat_err_euler(_destd_eu(_np(back2), c["st64"]), _destd_eu(c["x_eu"].numpy(), c["st64"])).max()
    gate = MARGIN * both
    print(f"[rotation] round trip aa -> euler -> aa: matrices {e1:.3e}; euler -> aa -> euler: matrices {e2:.3e}; gate {gate:.3e} "
          f"(= {MARGIN:g} x (eps_ref[fwd_mat] + eps_ref[inv_mat]))")
    assert torch.isfinite(back).all() and torch.isfinite(back2).all()
    assert e1 <= gate and e2 <= gate


# ---- 5. ragged ----------------------------------------------------------------------------------------------------------------------------
def test_ragged_lengths_zero_the_padded_rows_and_nothing_else():
    c = _fx()
    T, J = 17, c["J"]
    lens = [17, 5, 1]
    x_aa, x_eu = make_rotation_inputs(3, T, J, 77)
    calls = [("forward std", lambda t, **kw: glue.axis_angle_to_euler(t, c["stats"], **kw), x_aa),
             ("forward deg", lambda t, **kw: glue.axis_angle_to_euler(t, c["stats"], degrees=True, **kw), x_aa),
             ("inverse", lambda t, **kw: glue.euler_to_axis_angle(t, c["stats"], **kw), x_eu)]
    for name, fn, x in calls:
        full = fn(x.to(DEV))
        rag = fn(x.to(DEV), lengths=lens)
        dirty = x.clone()
        for b, n in enumerate(lens):
            dirty[b, n:] = float("nan")
            dirty[b, n::2] = 1e30
        rag_dirty = fn(dirty.to(DEV), lengths=torch.tensor(lens))
        for b, n in enumerate(lens):
            assert torch.equal(rag[b, :n], full[b, :n]), (name, b)
            assert int(torch.count_nonzero(rag[b, n:])) == 0 and not torch.isnan(rag[b, n:]).any(), (name, b)
        assert torch.equal(rag_dirty, rag), name
        assert float(full[1, 5:].abs().min()) > 0.0                # without lengths those rows do hold converted values
    # the wide tensor: gesture columns of the padded rows are zeros, the other columns come through as they are
    cfg = get_config("beat")
    wide = torch.cat([x_aa, torch.ones(3, T, cfg.expression_dim)], -1).to(DEV)
    out = glue.axis_angle_to_euler(wide, c["stats"], split_pos=cfg.split_pos, lengths=lens)
    assert int(torch.count_nonzero(out[1, 5:, :cfg.split_pos])) == 0 and torch.equal(out[..., cfg.split_pos:], wide[..., cfg.split_pos:])


# ---- 6. geometry independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [1, 47])
@pytest.mark.parametrize("wide", [False, True])
def test_rows_do_not_depend_on_the_launch_geometry(J, wide):
    stats = glue.PoseStats(**make_pose_stat_vectors(J, 5), device=DEV)
    g = torch.Generator().manual_seed(100 + J)
    for rows in (1, 2, 63, 64, 65, 257):
        x = torch.randn(rows, 192 if wide else 3 * J, generator=g).to(DEV)
        kw = {"split_pos": 3 * J} if wide else {}
        for fn in (glue.axis_angle_to_euler, glue.euler_to_axis_angle):
            whole = fn(x, stats, **kw)
            alone = torch.cat([fn(x[r:r + 1], stats, **kw) for r in range(rows)], 0)
            assert torch.isfinite(whole).all() and torch.equal(whole, alone), (fn.__name__, rows)
        if wide:                                                   # the stride changes nothing either
            assert torch.equal(fn(x, stats, **kw)[:, :3 * J], fn(x[:, :3 * J].contiguous(), stats))


# ---- 7. trainer ----------------------------------------------------------------------------------------------------------------------------------
def _beat_trainer():
    cfg = get_config("beat")
    return DDPMTrainer(sampler_namespace(cfg), gpu_model("beat", "fp32")), cfg


def _stream(cfg, B, N, seed):
    inp = make_inputs(cfg, B, frames=N, seed=seed)
    return inp["audio_emb"].to(DEV), inp["person_id"].to(DEV), {"pretrain_aud_feat": inp["pretrain_aud_feat"].to(DEV)}


@pytest.mark.parametrize("form", ["chain", "generate_batch", "lengths", "sharded"])
def test_trainer_pose_rep_is_the_conversion_of_the_default_result(form):
    c = _fx()
    tr, cfg = _beat_trainer()
    assert (cfg.n_poses, cfg.overlap_len) == (34, 4)
    if form == "chain":                                            # B = 2, N = 64: two windows
        a, pid, cond = _stream(cfg, 2, 64, 41)
        call = lambda **kw: tr.sample_arbitrary_len(a, pid, cond, seed=7, **kw)  # noqa: E731
    elif form == "generate_batch":
        a, pid, cond = _stream(cfg, 2, 34, 42)
        call = lambda **kw: tr.generate_batch(a, pid, cfg.net_dim_pose, cond, {}, seed=7, **kw)  # noqa: E731
    elif form == "lengths":
        a, pid, cond = _stream(cfg, 2, 64, 43)
        call = lambda **kw: tr.sample_arbitrary_len(a, pid, cond, seed=7, row_keys=[0, 1], lengths=[64, 41], **kw)  # noqa: E731
    else:                                                          # one stream, two chains, the seam between them re-sampled
        a, pid, cond = _stream(cfg, 1, 128, 44)
        call = lambda **kw: tr.sample_arbitrary_len_sharded(a, pid, cond, 2, seed=7, seam_repair=True, **kw)  # noqa: E731
    as_list = lambda r: list(r) if isinstance(r, (list, tuple)) else [r]  # noqa: E731
    with pytest.raises(ValueError):
        call(pose_rep="euler")                                     # no statistics yet
    before = as_list(call())
    tr.set_pose_stats(c["stats"])
    default = as_list(call())
    euler = as_list(call(pose_rep="euler"))
    assert len(before) == len(default) == len(euler) == (2 if form == "lengths" else 1)
    for b, d, e in zip(before, default, euler):
        assert torch.equal(b, d)                                   # the statistics alone change nothing
        want = glue.axis_angle_to_euler(d, c["stats"], split_pos=cfg.split_pos)
        assert e.shape == d.shape and torch.isfinite(e).all() and torch.equal(e, want)
        assert torch.equal(e[..., cfg.split_pos:], d[..., cfg.split_pos:]) and not torch.equal(e[..., :cfg.split_pos], d[..., :cfg.split_pos])
    if form == "lengths":
        assert [int(e.shape[0]) for e in euler] == [64, 41]
    if form == "generate_batch":                                   # ragged batch: padded frames stay 0 in the Euler result
        r = tr.generate_batch(a, pid, cfg.net_dim_pose, cond, {}, seed=7, lengths=[34, 20], pose_rep="euler")
        assert int(torch.count_nonzero(r[1, 20:])) == 0 and float(r[1, :20, :cfg.split_pos].abs().min()) > 0.0


# ---- 8. from_euler feeding sample_inbetween ------------------------------------------------------------------------------------------------------
def test_from_euler_feeds_sample_inbetween():
    """addBlend off and tail_blend off: every pinned frame of the result is the pinned value itself (with the fades only the first and
    the last frame carry weight 0).

    The statistics of this test are fitted to the clip, as a dataset's are to its poses: the synthetic weights make the sampler return
    standardised values of a few hundred (measured: mean |x| 230, max 1 340), which the fixture's statistics would turn into angles of
    hundreds of radians - and an fp32 angle of 390 rad carries half an ulp = 1.5e-5 rad of rounding in ANY implementation (measured with
    the fixture's statistics: 3.5e-5 as matrices on the forward leg alone, all of it on joints beyond 12 rad).  eps_ref describes
    standardised inputs of unit scale, so std_axis_angle is divided by the RMS of the clip's gesture channels; nothing else changes."""
    c = _fx()
    cfg = get_config("beat")
    tr = DDPMTrainer(sampler_namespace(cfg, addBlend=False), gpu_model("beat", "fp32"))
    L, S = cfg.overlap_len, cfg.split_pos
    a, pid, cond = _stream(cfg, 2, cfg.n_poses, 45)
    clip = tr.generate_batch(a, pid, cfg.net_dim_pose, cond, {}, seed=3)
    rms = float(clip[..., :S].square().mean().sqrt())
    st = dict(c["st"], std_axis_angle=c["st"]["std_axis_angle"] / rms)
    st64 = {k: v.double().numpy() for k, v in st.items()}
    stats = glue.PoseStats(**st, device=DEV)
    tr.set_pose_stats(stats)
    head, tail = clip[:, :L].contiguous(), clip[:, -L:].contiguous()
    head_e, tail_e = (glue.axis_angle_to_euler(t, stats, split_pos=S) for t in (head, tail))
    head_b, tail_b = tr.from_euler(head_e), tr.from_euler(tail_e.cpu())                  # (a host tensor is moved to the trainer's device)
    assert torch.equal(head_b[..., S:], head[..., S:]) and torch.equal(tail_b[..., S:], tail[..., S:])
    out = tr.sample_inbetween(a, pid, cond, head_b, tail_b, tail_blend=False, seed=11)
    assert torch.isfinite(out).all()
    assert torch.equal(out[:, :L], head_b) and torch.equal(out[:, -L:], tail_b)
    assert not torch.equal(out[:, L:-L], clip[:, L:-L])
    got = _destd_aa(_np(torch.cat([out[:, :L], out[:, -L:]], 1)[..., :S]), st64)
    want = _destd_aa(_np(torch.cat([head, tail], 1)[..., :S]), st64)
    e = _mat_err_aa(got, want).max()
    gate = MARGIN * (c["eps"]["fwd_mat"] + c["eps"]["inv_mat"])
    cos_y = np.abs(np.cos(np.radians(rr.joints(_destd_eu(_np(torch.cat([head_e, tail_e], 1)[..., :S]), st64))[..., 1]))).min()
    print(f"[rotation] from_euler: pinned frames against the original axis-angle frames, as matrices {e:.3e}, gate {gate:.3e} "
          f"(round-trip gate); clip RMS {rms:.1f}, largest angle {np.sqrt((rr.joints(want) ** 2).sum(-1)).max():.2f} rad, "
          f"smallest |cos Y| on the way {cos_y:.3e}")
    assert e <= gate
