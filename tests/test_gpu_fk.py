"""Forward kinematics on a real MI355X: ``dsh_fk_positions`` / ``dsh_fk_positions_vjp`` against the emulation of tests/fk_ref.py, their
geometry and ragged rules bit for bit, every refusal through C and Python, and ``return_positions`` of the sampling entry points.

Tolerances: no number is fixed here.  Truth is the emulation in float64 (forward) and float64 autograd through it (VJP).  Every gate is
MARGIN x eps_ref, eps_ref being the error of the SAME emulation run in float32 (for the VJP: float32 autograd) on the same inputs, per
skeleton; MARGIN = 4 covers a different but equally valid fp32 operation order and the device's sinf / cosf.  Positions are normalised
by the skeleton's total bone length, world rotations are compared as matrices, gradients are normalised by the largest entry of the
truth.  tests/test_fk_cpu.py shows that these gates reject the five classic mistakes on these inputs.

Measured on an MI355X (error / eps_ref at 257 rows; the gate is 4; positions, rotations, gradient): single 0 (exact), 0.69, 0 (exact);
chain3 0.67, 0.69, 1.10; tree7 1.00, 0.84, 0.99; rand90 0.90, 1.00, 1.21; big256 1.14, 0.91, 1.35."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fk_ref as fk  # noqa: E402
from diffsheg_amd import _lib, glue  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.streaming import StreamPool  # noqa: E402
from diffsheg_amd.synthetic import make_inputs, make_pose_stat_vectors  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from util import gpu_model  # noqa: E402

DEV = "cuda:0"
_DEVICE = {}


def _dev(name):
    """The device side of a case, uploaded once: skeleton buffers, statistics, inputs tight and wide, cotangents."""
    if name not in _DEVICE:
        c = fk.case(name)
        sk = c["sk"]
        skel = glue.Skeleton(sk["parents"], sk["offsets"], sk["channel_joint"], rest=sk["rest_deg"])
        assert np.abs(skel.rest_rot - sk["rest_rot"]).max() < 1e-15 and abs(skel.bone_length - sk["bone_length"]) < 1e-9
        n = 3 * c["Jc"]
        ld = 192 if n <= 192 - 8 else n + 8                       # the wide form: BEAT's row where the channels fit, else 8 spare columns
        x = torch.from_numpy(c["x"])
        wide = torch.full((x.shape[0], ld), float("nan"))          # what lies behind the channels is never read
        wide[:, :n] = x
        zeros = torch.zeros(n)
        stats = glue.PoseStats(torch.from_numpy(c["mean"]), torch.from_numpy(c["std"]), zeros, zeros + 1.0, device=DEV)
        _DEVICE[name] = dict(c=c, skel=skel, bufs=skel.to(DEV), stats=stats, x=x.to(DEV), wide=wide.to(DEV), ld=ld,
                             g=torch.from_numpy(c["g"]).reshape(x.shape[0], -1).to(DEV))
    return _DEVICE[name]


def _ptr(t):
    return t if t is None or isinstance(t, int) else t.data_ptr()


def _skel_args(d, **over):
    b, c = d["bufs"], d["c"]
    a = dict(joints=c["J"], channels=c["Jc"], parents=_ptr(b["parents"]), offsets=_ptr(b["offsets"]), channel_joint=_ptr(b["channel_joint"]),
             rest_rot=_ptr(b["rest_rot"]), joint_channel=_ptr(b["joint_channel"]))
    a.update(over)
    return [a[k] for k in ("joints", "channels", "parents", "offsets", "channel_joint", "rest_rot", "joint_channel")]


def c_forward(d, x, rows, ld, lengths=None, frames=0, want_wrot=True, kind=0, rc_only=False, **over):
    """dsh_fk_positions on the first `rows` rows of x (stride ld); outputs prefilled with NaN so that an unwritten element shows"""
    J = d["c"]["J"]
    pos = torch.full((max(rows, 1), 3 * J), float("nan"), device=DEV)        # (at least a row: an empty tensor has a null pointer)
    wrot = torch.full((max(rows, 1), 9 * J), float("nan"), device=DEV) if want_wrot else None
    a = dict(x=_ptr(x), ld=ld, rows=rows, kind=kind, mean=_ptr(d["stats"].mean_axis_angle), std=_ptr(d["stats"].std_axis_angle),
             pos=_ptr(pos), ld_pos=3 * J, wrot=_ptr(wrot), ld_wrot=9 * J, lengths=_ptr(lengths), frames=frames)
    skel_over = {k: over.pop(k) for k in list(over) if k not in a}
    a.update(over)
    rc = _lib.lib().dsh_fk_positions(None, a["x"], a["ld"], a["rows"], a["kind"], a["mean"], a["std"], *_skel_args(d, **skel_over),
                                     a["pos"], a["ld_pos"], a["wrot"], a["ld_wrot"], a["lengths"], a["frames"])
    if rc_only:
        return rc
    _lib.check(rc, "dsh_fk_positions")
    return pos[:rows], (wrot[:rows] if want_wrot else None)


def c_vjp(d, x, g, rows, ld, lengths=None, frames=0, kind=0, rc_only=False, **over):
    J, n = d["c"]["J"], 3 * d["c"]["Jc"]
    dx = torch.full((max(rows, 1), n), float("nan"), device=DEV)
    a = dict(x=_ptr(x), ld=ld, rows=rows, kind=kind, mean=_ptr(d["stats"].mean_axis_angle), std=_ptr(d["stats"].std_axis_angle),
             g=_ptr(g), ld_g=3 * J, dx=_ptr(dx), ld_dx=n, lengths=_ptr(lengths), frames=frames)
    skel_over = {k: over.pop(k) for k in list(over) if k not in a}
    a.update(over)
    rc = _lib.lib().dsh_fk_positions_vjp(None, a["x"], a["ld"], a["rows"], a["kind"], a["mean"], a["std"], *_skel_args(d, **skel_over),
                                         a["g"], a["ld_g"], a["dx"], a["ld_dx"], a["lengths"], a["frames"])
    if rc_only:
        return rc
    _lib.check(rc, "dsh_fk_positions_vjp")
    return dx[:rows]


def _gate(what, got, eps, name):
    gate = fk.MARGIN * eps
    ratio = got / eps if eps > 0 else (0.0 if got == 0 else float("inf"))
    print(f"[fk] {what}: measured {got:.3e}, eps_ref {eps:.3e}, ratio {ratio:.2f} (gate {fk.MARGIN:g})")
    assert np.isfinite(got) and got <= gate, (what, got, gate)


# ---- 1. forward -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fk.SKELETONS)
def test_forward_against_the_float64_emulation(name):
    d = _dev(name)
    c = d["c"]
    for rows in fk.ROW_COUNTS:
        pos, wrot = c_forward(d, d["x"], rows, 3 * c["Jc"])
        pos_w, wrot_w = c_forward(d, d["wide"], rows, d["ld"])
        assert torch.isfinite(pos).all() and torch.isfinite(wrot).all()
        assert torch.equal(pos, pos_w) and torch.equal(wrot, wrot_w)                       # the stride changes nothing
        pos_only, none = c_forward(d, d["x"], rows, 3 * c["Jc"], want_wrot=False)
        assert none is None and torch.equal(pos_only, pos)                                 # nor does leaving the rotations out
        e_pos, e_rot = fk.forward_errors(pos.cpu(), wrot.cpu(), c)
        _gate(f"{name} rows {rows} positions / bone length", e_pos, c["eps"]["pos"], name)
        _gate(f"{name} rows {rows} world rotations as matrices", e_rot, c["eps"]["wrot"], name)
    # through Python: the same bits, in the public shapes
    p, w = glue.joint_positions(d["wide"], d["skel"], d["stats"], split_pos=3 * c["Jc"], world_rotations=True)
    assert p.shape == (257, c["J"], 3) and w.shape == (257, c["J"], 3, 3)
    assert torch.equal(p.reshape(257, -1), pos) and torch.equal(w.reshape(257, -1), wrot)
    assert torch.equal(glue.joint_positions(d["x"], d["skel"], d["stats"]), p)


def test_forward_known_answer_chain():
    """Quarter turns on the unit chain: the positions are integers.  Held to the float64 truth at MARGIN x the float32 emulation's own
    error on these rows, as every other case."""
    d = _dev("chain3")
    sk = d["c"]["sk"]
    q = np.pi / 2
    v = np.array([[0, 0, q, 0, 0, q, 0, 0, q], [0, 0, q, 0, 0, -q, 0, 0, 0], [0, q, 0, 0, 0, q, 0, 0, 0]])
    mean, std = d["c"]["mean"], d["c"]["std"]
    x = ((v - mean.astype(np.float64)) / std.astype(np.float64)).astype(np.float32)
    with torch.no_grad():
        p64, w64 = fk.forward(x, sk, mean, std, torch.float64)
        p32, w32 = fk.forward(x, sk, mean, std, torch.float32)
    want = np.array([[[0, 0, 0], [0, 1, 0], [-1, 1, 0]], [[0, 0, 0], [0, 1, 0], [1, 1, 0]], [[0, 0, 0], [0, 0, -1], [0, 1, -1]]], dtype=np.float64)
    assert np.abs(p64.numpy() - want).max() < 1e-6                 # (x is a float32: the angles are quarter turns to 1e-7)
    pos, wrot = c_forward(d, torch.from_numpy(x).to(DEV), 3, 9)
    e_pos = float((pos.cpu().double().reshape(3, 3, 3) - p64).abs().max()) / sk["bone_length"]
    e_rot = float((wrot.cpu().double().reshape(3, 3, 3, 3) - w64).abs().max())
    _gate("known-answer chain positions / bone length", e_pos, float((p32.double() - p64).abs().max()) / sk["bone_length"], "chain3")
    _gate("known-answer chain world rotations", e_rot, float((w32.double() - w64).abs().max()), "chain3")
    assert np.abs(pos.cpu().numpy().reshape(3, 3, 3) - want).max() < 1e-6


def test_forward_euler_input():
    """kind = 1 on the Euler form of the same rotations: the positions of the axis-angle run, to both runs' float32 yardsticks."""
    d = _dev("tree7")
    c = d["c"]
    sk, Jc = c["sk"], c["Jc"]
    rng = np.random.RandomState(8)
    deg = rng.uniform(-180, 180, size=(33, 3 * Jc))
    deg[:, 1::3] = rng.uniform(-80, 80, size=(33, Jc))
    mean_e, std_e = (15 * rng.normal(size=3 * Jc)).astype(np.float32), rng.uniform(3, 30, size=3 * Jc).astype(np.float32)
    x = ((deg - mean_e.astype(np.float64)) / std_e.astype(np.float64)).astype(np.float32)
    with torch.no_grad():
        p64, w64 = fk.forward(x, sk, mean_e, std_e, torch.float64, kind="euler")
        p32, w32 = fk.forward(x, sk, mean_e, std_e, torch.float32, kind="euler")
    stats = glue.PoseStats(torch.zeros(3 * Jc), torch.ones(3 * Jc), torch.from_numpy(mean_e), torch.from_numpy(std_e), device=DEV)
    pos, wrot = glue.joint_positions(torch.from_numpy(x).to(DEV), d["skel"], stats, kind="euler", world_rotations=True)
    _gate("euler input positions / bone length", float((pos.cpu().double() - p64).abs().max()) / sk["bone_length"],
          float((p32.double() - p64).abs().max()) / sk["bone_length"], "tree7")
    _gate("euler input world rotations", float((wrot.cpu().double() - w64).abs().max()), float((w32.double() - w64).abs().max()), "tree7")


# ---- 2. VJP ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fk.SKELETONS)
def test_vjp_against_float64_autograd(name):
    d = _dev(name)
    c = d["c"]
    n = 3 * c["Jc"]
    for rows in fk.ROW_COUNTS:
        dx = c_vjp(d, d["x"], d["g"], rows, n)
        assert torch.isfinite(dx).all()
        assert torch.equal(dx, c_vjp(d, d["wide"], d["g"], rows, d["ld"]))
        _gate(f"{name} rows {rows} gradient / largest entry", fk.vjp_error(dx.cpu(), c), c["eps"]["vjp"], name)
    # rows 1 and 3: the cotangent is zero except on the last joint, a leaf - only its ancestors' channels see it, the others are exactly 0
    anc = set(fk.ancestors(c["sk"], c["J"] - 1))
    got = dx.cpu().reshape(257, c["Jc"], 3)
    for r in (1, 3):
        for i, j in enumerate(c["sk"]["channel_joint"]):
            if int(j) in anc:
                assert bool((got[r, i] != 0).all()), (name, r, i)
            else:
                assert int(torch.count_nonzero(got[r, i])) == 0, (name, r, i)
    # torch.autograd through the public call is this very launch
    xw = d["wide"].clone().requires_grad_(True)
    pos = glue.joint_positions(xw, d["skel"], d["stats"], split_pos=n)
    pos.backward(d["g"].reshape(pos.shape))
    assert torch.equal(xw.grad[:, :n], dx) and int(torch.count_nonzero(xw.grad[:, n:])) == 0
    xt = d["x"].clone().requires_grad_(True)
    p, w = glue.joint_positions(xt, d["skel"], d["stats"], world_rotations=True)
    assert not w.requires_grad
    (gx,) = torch.autograd.grad(p, xt, d["g"].reshape(p.shape))
    assert torch.equal(gx, dx)


def test_a_torch_optimiser_moves_a_pose_towards_a_target():
    d = _dev("tree7")
    target = glue.joint_positions(d["x"][5:6], d["skel"], d["stats"])
    pose = d["x"][9:10].clone().requires_grad_(True)
    opt = torch.optim.SGD([pose], lr=2e-4)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = (glue.joint_positions(pose, d["skel"], d["stats"]) - target).square().sum()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print("[fk] SGD on a pose, position loss per step:", ["%.4f" % v for v in losses])
    assert all(b < a for a, b in zip(losses, losses[1:]))
    total = glue.joint_positions(d["x"][:3].clone().requires_grad_(True), d["skel"], d["stats"]).sum()
    total.backward()                                              # pos.sum().backward() works: the cotangent is an expanded scalar


# ---- 3. geometry independence -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fk.SKELETONS)
def test_rows_do_not_depend_on_the_launch_geometry(name):
    d = _dev(name)
    c = d["c"]
    n, J = 3 * c["Jc"], c["J"]
    pos, wrot = c_forward(d, d["x"], 257, n)
    dx = c_vjp(d, d["x"], d["g"], 257, n)
    for rows in (1, 2, 3, 4, 5, 63, 64, 65):                        # a prefix run is the same rows in another grid
        p, w = c_forward(d, d["x"], rows, n)
        assert torch.equal(p, pos[:rows]) and torch.equal(w, wrot[:rows]) and torch.equal(c_vjp(d, d["x"], d["g"], rows, n), dx[:rows]), rows
    alone_p, alone_w, alone_dx = [], [], []
    for r in range(257):                                            # every row alone
        p, w = c_forward(d, d["x"][r:r + 1], 1, n)
        alone_p.append(p)
        alone_w.append(w)
        alone_dx.append(c_vjp(d, d["x"][r:r + 1], d["g"][r:r + 1], 1, n))
    assert torch.equal(torch.cat(alone_p), pos) and torch.equal(torch.cat(alone_w), wrot) and torch.equal(torch.cat(alone_dx), dx)


# ---- 4. ragged -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tree7", "rand90"])
def test_ragged_lengths_zero_the_padded_rows_and_never_read_them(name):
    d = _dev(name)
    c = d["c"]
    n, J, frames = 3 * c["Jc"], c["J"], 5
    lens = [frames, 1, 3]
    rows = 3 * frames
    x, g = d["x"][:rows].clone(), d["g"][:rows].clone()
    pos, wrot = c_forward(d, x, rows, n)
    dx = c_vjp(d, x, g, rows, n)
    xd, gd = x.clone().view(3, frames, n), g.clone().view(3, frames, 3 * J)
    for b, L in enumerate(lens):
        xd[b, L:] = float("nan")
        gd[b, L:] = float("nan")
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    rp, rw = c_forward(d, xd, rows, n, lengths=lens_dev, frames=frames)
    rdx = c_vjp(d, xd, gd, rows, n, lengths=lens_dev, frames=frames)
    for got, full in ((rp, pos), (rw, wrot), (rdx, dx)):
        got, full = got.view(3, frames, -1), full.view(3, frames, -1)
        for b, L in enumerate(lens):
            assert torch.equal(got[b, :L], full[b, :L]), (name, b)
            assert int(torch.count_nonzero(got[b, L:])) == 0 and not torch.isnan(got[b, L:]).any(), (name, b)
    # through Python, forward and backward
    xp = xd.clone().requires_grad_(True)
    p = glue.joint_positions(xp, d["skel"], d["stats"], lengths=lens)
    assert p.shape == (3, frames, J, 3) and torch.equal(p.reshape(rows, -1), rp)
    p.backward(gd.view(3, frames, J, 3))
    assert torch.equal(xp.grad.view(rows, n), rdx)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_through_c():
    d = _dev("tree7")
    c = d["c"]
    n, J = 3 * c["Jc"], c["J"]
    lens_dev = torch.tensor([2, 2], dtype=torch.int32, device=DEV)
    bad = [dict(x=None), dict(mean=None), dict(std=None), dict(parents=None), dict(offsets=None), dict(channel_joint=None),
           dict(rest_rot=None), dict(joint_channel=None), dict(ld=n - 1), dict(rows=-1), dict(joints=0), dict(joints=257),
           dict(channels=0), dict(channels=J + 1), dict(kind=2), dict(lengths=_ptr(lens_dev), frames=0), dict(lengths=_ptr(lens_dev), frames=3)]
    for kw in bad + [dict(pos=None), dict(ld_pos=3 * J - 1), dict(ld_wrot=9 * J - 1)]:
        assert c_forward(d, rc_only=True, **dict(dict(x=d["x"], rows=4, ld=n), **kw)) == -1, kw
        assert _lib.lib().dsh_last_error()
    for kw in bad + [dict(g=None), dict(dx=None), dict(ld_g=3 * J - 1), dict(ld_dx=n - 1), dict(kind=1)]:
        assert c_vjp(d, rc_only=True, **dict(dict(x=d["x"], g=d["g"], rows=4, ld=n), **kw)) == -1, kw
    # a null rotation output with any stride is no refusal; nor are zero rows; nor kind 1 forward
    assert c_forward(d, d["x"], 4, n, rc_only=True, wrot=None, ld_wrot=0) == 0
    assert c_forward(d, d["x"], 0, n, rc_only=True) == 0 and c_vjp(d, d["x"], d["g"], 0, n, rc_only=True) == 0
    assert c_forward(d, d["x"], 4, n, rc_only=True, kind=1) == 0
    assert c_forward(d, d["x"], 4, n, rc_only=True, lengths=_ptr(lens_dev), frames=2) == 0
    torch.cuda.synchronize()


def test_refusals_through_python():
    d = _dev("tree7")
    c = d["c"]
    n = 3 * c["Jc"]
    x, sk, st = d["x"][:6], d["skel"], d["stats"]
    small = glue.PoseStats(*[torch.ones(n - 3)] * 4, device=DEV)
    for call in (lambda: glue.joint_positions(x, "skeleton", st), lambda: glue.joint_positions(x, sk, None),
                 lambda: glue.joint_positions(x, sk, st, kind="quaternion"), lambda: glue.joint_positions(x[:, :n - 3], sk, small),
                 lambda: glue.joint_positions(x, sk, st, split_pos=n - 3), lambda: glue.joint_positions(x, sk, small),
                 lambda: glue.joint_positions(x, sk, st, lengths=[3, 3]), lambda: glue.joint_positions(x.view(2, 3, n), sk, st, lengths=[3, 4]),
                 lambda: glue.joint_positions(x.view(2, 3, n), sk, st, lengths=[0, 3]), lambda: glue.joint_positions(x[0, 0], sk, st),
                 lambda: glue.joint_positions(x.clone().requires_grad_(True), sk, st, kind="euler")):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(_lib.DshError):
        glue.joint_positions(x.cpu(), sk, st)
    with torch.no_grad():                                          # no gradient is requested here: kind "euler" runs
        assert glue.joint_positions(x.clone().requires_grad_(True), sk, st, kind="euler").shape == (6, c["J"], 3)


# ---- 6. model level ---------------------------------------------------------------------------------------------------------------------------------------------
def _beat():
    cfg = get_config("beat")
    tr = DDPMTrainer(sampler_namespace(cfg), gpu_model("beat", "fp32"))
    skel = _dev("rand90")["skel"]
    assert 3 * skel.channels == cfg.split_pos
    stats = glue.PoseStats(**make_pose_stat_vectors(skel.channels, 21), device=DEV)
    return tr, cfg, skel, stats


def _stream(cfg, B, N, seed):
    inp = make_inputs(cfg, B, frames=N, seed=seed)
    return inp["audio_emb"].to(DEV), inp["person_id"].to(DEV), {"pretrain_aud_feat": inp["pretrain_aud_feat"].to(DEV)}


def test_generate_batch_return_positions():
    tr, cfg, skel, stats = _beat()
    a, pid, cond = _stream(cfg, 2, cfg.n_poses, 42)
    call = lambda **kw: tr.generate_batch(a, pid, cfg.net_dim_pose, cond, {}, seed=7, **kw)  # noqa: E731
    before = call()
    with pytest.raises(ValueError):
        call(return_positions=True)                                # no statistics
    with pytest.raises(ValueError):
        tr.set_skeleton(skel)                                      # set_skeleton needs them too
    tr.set_pose_stats(stats)
    with pytest.raises(ValueError):
        call(return_positions=True)                                # no skeleton
    with pytest.raises(ValueError):
        tr.set_skeleton(_dev("tree7")["skel"])                     # not the gesture channels' 47 joints
    tr.set_skeleton(skel)
    result, pos = call(return_positions=True)
    assert torch.equal(result, before) and torch.equal(call(), before)
    assert pos.shape == (2, cfg.n_poses, skel.joints, 3) and torch.isfinite(pos).all()
    assert torch.equal(pos, tr.joint_positions(result))
    assert torch.equal(pos, glue.joint_positions(result, skel, stats, split_pos=cfg.split_pos))
    # with pose_rep="euler" the positions still come from the axis-angle result
    e, pos_e = call(return_positions=True, pose_rep="euler")
    assert torch.equal(e, call(pose_rep="euler")) and torch.equal(pos_e, pos)
    # ragged: padded frames of the positions are 0
    r, pr = call(return_positions=True, lengths=[cfg.n_poses, 20])
    assert torch.equal(r, call(lengths=[cfg.n_poses, 20])) and int(torch.count_nonzero(pr[1, 20:])) == 0
    assert torch.equal(pr[1, :20], tr.joint_positions(r[1, :20]))
    # SHOW, and BEAT without axis-angle channels, are refused
    show = DDPMTrainer(sampler_namespace(get_config("show")), gpu_model("show", "fp32"))
    show.pose_stats, show.skeleton = stats, skel
    with pytest.raises(ValueError):
        show._positions_requested(True)
    tr.opt.axis_angle = False
    with pytest.raises(ValueError):
        call(return_positions=True)


def test_chain_and_stream_pool_return_positions():
    tr, cfg, skel, stats = _beat()
    tr.set_pose_stats(stats)
    tr.set_skeleton(skel)
    N = 2 * cfg.n_poses - cfg.overlap_len                          # two windows
    a, pid, cond = _stream(cfg, 2, N, 41)
    chain = lambda **kw: tr.sample_arbitrary_len(a, pid, cond, seed=7, **kw)  # noqa: E731
    full, pos = chain(return_positions=True)
    assert torch.equal(full, chain()) and pos.shape == (2, N, skel.joints, 3) and torch.equal(pos, tr.joint_positions(full))
    lens = [N, cfg.n_poses + 7]
    outs, poss = chain(return_positions=True, row_keys=[0, 1], lengths=lens)
    plain = chain(row_keys=[0, 1], lengths=lens)
    assert [int(p.shape[0]) for p in poss] == lens
    for o, q, p in zip(outs, plain, poss):
        assert torch.equal(o, q) and torch.equal(p, tr.joint_positions(o))
    # a live session: the positions of the frames one stride emits
    pools = [StreamPool(tr, 1, 9) for _ in range(2)]
    got = []
    for pool, kw in zip(pools, ({}, {"return_positions": True})):
        sid = pool.open(pid[0], key=3)
        pool.feed(sid, a[0, :cfg.n_poses], {"pretrain_aud_feat": cond["pretrain_aud_feat"][0, :cfg.n_poses]})
        got.append((sid, pool.step(**kw)))
    (sid0, frames0), (sid1, (frames1, pos1)) = got
    assert torch.equal(frames1[sid1], frames0[sid0]) and pos1[sid1].shape == (cfg.n_poses - cfg.overlap_len, skel.joints, 3)
    assert torch.equal(pos1[sid1], tr.joint_positions(frames1[sid1]))
    assert pools[1].step(return_positions=True) == ({}, {})
    rest, rest_pos = pools[1].close(sid1, return_positions=True)
    assert torch.equal(rest, pools[0].close(sid0)) and torch.equal(rest_pos, tr.joint_positions(rest))


def test_empty_batches_give_empty_results_without_a_call():
    """Zero rows: an empty tensor's pointer is null, which the C calls refuse - Python returns the empty results itself."""
    d = _dev("tree7")
    c = d["c"]
    n, J = 3 * c["Jc"], c["J"]
    for shape in ((0, n), (0, 192), (2, 0, n), (0, 5, n)):
        kw = {"split_pos": n} if shape[-1] != n else {}
        x = torch.empty(shape, device=DEV)
        p, w = glue.joint_positions(x, d["skel"], d["stats"], world_rotations=True, **kw)
        assert p.shape == shape[:-1] + (J, 3) and w.shape == shape[:-1] + (J, 3, 3) and p.is_cuda
        assert glue.joint_positions(x, d["skel"], d["stats"], kind="euler", **kw).shape == shape[:-1] + (J, 3)
        xg = x.clone().requires_grad_(True)
        glue.joint_positions(xg, d["skel"], d["stats"], **kw).sum().backward()
        assert xg.grad.shape == shape and xg.grad.numel() == 0


def test_closing_sessions_that_owe_nothing_with_return_positions():
    """close / close_many with return_positions on sessions of zero frames, alone and beside sessions that owe frames: ``[0, C]`` frames
    and ``[0, J, 3]`` positions, the slot is freed, and the others' frames and positions are those of the call without the keyword."""
    tr, cfg, skel, stats = _beat()
    tr.set_pose_stats(stats)
    tr.set_skeleton(skel)
    J, Cc, L = skel.joints, cfg.net_dim_pose, cfg.overlap_len
    a, pid, cond = _stream(cfg, 2, cfg.n_poses + 7, 46)
    hub = cond["pretrain_aud_feat"]
    # a session opened and never fed, alone
    pool = StreamPool(tr, 1, 9)
    sid = pool.open(pid[0])
    frames, pos = pool.close(sid, return_positions=True)
    assert frames.shape == (0, Cc) and pos.shape == (0, J, 3) and pos.is_cuda and len(pool) == 0
    sid = pool.open(pid[0])                                        # the slot came back
    frames, pos = pool.close(sid, pose_rep="euler", return_positions=True)
    assert frames.shape == (0, Cc) and pos.shape == (0, J, 3) and len(pool) == 0
    out, poss = pool.close_many([pool.open(pid[0])], return_positions=True)
    assert [tuple(t.shape) for t in out.values()] == [(0, Cc)] and [tuple(t.shape) for t in poss.values()] == [(0, J, 3)]
    # mixed: one unfed, one with a window and a tail, one short - against the same pool without the keyword
    res = []
    for kw in ({}, {"return_positions": True}, {"return_positions": True, "pose_rep": "euler"}):
        pool = StreamPool(tr, 3, 9)
        s_empty, s_long, s_short = pool.open(pid[0], key=10), pool.open(pid[1], key=11), pool.open(pid[0], key=12)
        pool.feed(s_long, a[1], {"pretrain_aud_feat": hub[1]})
        pool.feed(s_short, a[0, :20], {"pretrain_aud_feat": hub[0, :20]})
        res.append(((s_empty, s_long, s_short), pool.close_many([s_empty, s_long, s_short], **kw)))
        assert len(pool) == 0
    (sids, plain), (_, (frames, pos)), (_, (frames_e, pos_e)) = res
    s_empty, s_long, s_short = sids
    assert set(frames) == set(pos) == set(plain) == set(sids)
    assert [int(plain[s].shape[0]) for s in sids] == [0, cfg.n_poses + 7, 20]
    euler_plain = tr._to_euler(torch.cat([plain[s_long], plain[s_short]], 0))
    for s in sids:
        assert torch.equal(frames[s], plain[s]) and pos[s].shape == (int(plain[s].shape[0]), J, 3)
        assert torch.equal(pos[s], tr.joint_positions(plain[s])) and torch.equal(pos_e[s], pos[s])
    assert frames_e[s_empty].shape == (0, Cc)
    assert torch.equal(torch.cat([frames_e[s_long], frames_e[s_short]], 0), euler_plain)


def test_position_metrics_on_the_device():
    d = _dev("rand90")
    pos = glue.joint_positions(d["x"][:12].view(2, 6, -1), d["skel"], d["stats"])
    same = glue.position_metrics(pos, pos, pck_threshold=1e-3)
    assert same["mpjpe"].is_cuda and same["mpjpe"].dim() == 0
    assert float(same["mpjpe"]) == 0.0 and float(same["pck"]) == 1.0
    shifted = pos + torch.tensor([0.0, 3.0, 4.0], device=DEV)      # every joint 5 away
    m = glue.position_metrics(pos, shifted, pck_threshold=6.0)
    assert abs(float(m["mpjpe"]) - 5.0) < 1e-4 and float(m["pck"]) == 1.0
    assert float(glue.position_metrics(pos, shifted, pck_threshold=4.0)["pck"]) == 0.0
    shifted[1, 4:] = float("nan")
    m = glue.position_metrics(pos, shifted, lengths=[6, 4], pck_threshold=6.0)
    assert abs(float(m["mpjpe"]) - 5.0) < 1e-4 and float(m["pck"]) == 1.0
