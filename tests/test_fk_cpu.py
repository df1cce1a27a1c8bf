"""Forward kinematics without a GPU: the emulation (tests/fk_ref.py) on known answers and against the rotation fixture, its hand-written VJP
against torch autograd, ``glue.Skeleton`` validation and the BVH header reader, and the proof that the GPU gates (MARGIN x the float32
emulation's own error, tests/test_gpu_fk.py) reject the five classic mistakes on the GPU tests' own inputs."""
import numpy as np
import pytest
import torch

import fk_ref as fk
from diffsheg_amd import glue
from diffsheg_amd.synthetic import make_pose_stat_vectors, make_rotation_inputs
from util import golden

F64 = torch.float64


def _unit(Jc):
    return np.zeros(3 * Jc, np.float32), np.ones(3 * Jc, np.float32)


# ---- known answers ------------------------------------------------------------------------------------------------------------------------
def test_planar_chain_with_right_angles_lands_on_integers():
    sk = fk.skeleton("chain3")
    mean, std = _unit(3)
    q = np.pi / 2
    x = np.array([[0, 0, q, 0, 0, q, 0, 0, q],            # three quarter turns about z
                  [0, 0, q, 0, 0, -q, 0, 0, 0],           # a quarter turn and back
                  [0, q, 0, 0, 0, q, 0, 0, 0]])           # about y, then about the turned z
    pos, wrot = fk.forward(x, sk, mean, std, F64)
    want = np.array([[[0, 0, 0], [0, 1, 0], [-1, 1, 0]],
                     [[0, 0, 0], [0, 1, 0], [1, 1, 0]],
                     [[0, 0, 0], [0, 0, -1], [0, 1, -1]]], dtype=np.float64)
    assert np.abs(pos.numpy() - want).max() < 1e-15
    assert np.abs(wrot[0, 2].numpy() - np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]])).max() < 1e-15        # Rz(270)
    assert np.abs(wrot[1, 1].numpy() - np.eye(3)).max() < 1e-15


def test_single_root_sits_at_its_offset():
    sk = fk.skeleton("single")
    mean, std = fk.statistics(1, 3)
    pos, wrot = fk.forward(fk.inputs(1, 4, 5, mean, std), sk, mean, std, F64)
    assert torch.equal(pos, torch.tensor([1.0, 2.0, 3.0], dtype=F64).expand(4, 1, 3))
    v = fk.denormalise(fk.inputs(1, 4, 5, mean, std), sk, mean, std, F64)
    assert torch.equal(wrot[:, 0], fk.aa_matrices(v)[:, 0])


def test_undriven_joint_keeps_its_rest_rotation():
    sk = fk._skeleton([-1, 0, 1], [[0, 0, 0], [1, 0, 0], [1, 0, 0]], [0], rest=[[0, 0, 0], [0, 0, 90.0], [0, 0, 0]])
    mean, std = _unit(1)
    pos, wrot = fk.forward(np.zeros((1, 3)), sk, mean, std, F64)
    # the root is at rest; joint 1 turns its child's bone a quarter about z: (1, 0, 0) + Rz(90) (1, 0, 0) = (1, 1, 0)
    assert np.abs(pos[0].numpy() - np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])).max() < 1e-15
    assert np.abs(wrot[0, 1].numpy() - np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]])).max() < 1e-15
    off, _ = fk.forward(np.zeros((1, 3)), sk, mean, std, F64, mutant="rest_ignored")
    assert np.abs(off[0, 2].numpy() - np.array([2.0, 0, 0])).max() < 1e-15


# ---- Euler input against axis-angle input on the rotation fixture -----------------------------------------------------------------------------
def test_euler_input_gives_the_positions_of_the_axis_angle_input():
    f = golden("rotations_beat.npz")
    B, T, J = int(f["batch"]), int(f["frames"]), int(f["joints"])
    st = make_pose_stat_vectors(J, int(f["stats_seed"]))
    x_aa, _ = make_rotation_inputs(B, T, J, int(f["input_seed"]))
    # a star: an undriven root, every driven joint its child, each with an end site - end site i moves with joint i alone
    rng = np.random.RandomState(4)
    parents = [-1] + [0] * J + list(range(1, J + 1))
    sk = fk._skeleton(parents, rng.uniform(-5, 5, size=(2 * J + 1, 3)), list(range(1, J + 1)))
    rows = B * T
    p_aa, _ = fk.forward(x_aa.reshape(rows, 3 * J).numpy(), sk, st["mean_axis_angle"].numpy(), st["std_axis_angle"].numpy(), F64)
    p_eu, _ = fk.forward(f["euler_deg_f64"].reshape(rows, 3 * J), sk, *(a.astype(np.float64) for a in _unit(J)), F64, kind="euler")
    wc = f["well_conditioned"].reshape(rows, J)
    assert wc.mean() > 0.8
    err = (p_aa[:, J + 1:] - p_eu[:, J + 1:]).abs().max(-1).values.numpy() / sk["bone_length"]
    print(f"[fk] euler vs axis-angle input, end sites of well-conditioned joints: {err[wc].max():.3e} of the bone length")
    assert err[wc].max() < 1e-12
    assert torch.equal(p_aa[:, :J + 1], p_eu[:, :J + 1])          # the root and the joints themselves do not move at all


# ---- the hand-written VJP against autograd ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["single", "chain3", "tree7", "rand90"])
def test_emulated_vjp_is_autograd_of_the_emulation(name):
    c = fk.case(name)
    n = 9
    got = fk.vjp(c["x"][:n], c["g"][:n], c["sk"], c["mean"], c["std"], F64)
    want = c["grad64"][:n]
    rel = float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)
    print(f"[fk] {name}: emulated VJP against float64 autograd {rel:.3e}")
    assert rel <= 1e-10
    if name != "single":
        assert float(want.abs().max()) > 0.0


def test_leaf_only_cotangent_reaches_the_ancestors_only():
    c = fk.case("rand90")
    sk = c["sk"]
    anc = set(fk.ancestors(sk, c["J"] - 1))
    got = fk.vjp(c["x"][:4], c["g"][:4], sk, c["mean"], c["std"], F64).reshape(4, c["Jc"], 3)
    for r in (1, 3):
        for i, j in enumerate(sk["channel_joint"]):
            assert bool((got[r, i] != 0).all()) == (int(j) in anc), (r, i, j)
    assert any(int(j) in anc for j in sk["channel_joint"])


# ---- the gates reject the classic mistakes, on the GPU tests' inputs -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tree7", "rand90"])
@pytest.mark.parametrize("mutant", fk.FORWARD_MUTANTS)
def test_forward_gates_reject(name, mutant):
    c = fk.case(name)
    with torch.no_grad():
        pos, wrot = fk.forward(c["x"], c["sk"], c["mean"], c["std"], F64, mutant=mutant)
    e_pos, e_rot = fk.forward_errors(pos, wrot, c)
    print(f"[fk] {name} / {mutant}: positions {e_pos:.3e} (gate {fk.MARGIN * c['eps']['pos']:.3e}), rotations {e_rot:.3e} "
          f"(gate {fk.MARGIN * c['eps']['wrot']:.3e})")
    assert c["eps"]["pos"] > 0 and c["eps"]["wrot"] > 0
    assert e_pos > fk.MARGIN * c["eps"]["pos"]
    if mutant != "offset_by_own_rotation":                       # (that one leaves the rotations right)
        assert e_rot > fk.MARGIN * c["eps"]["wrot"]


@pytest.mark.parametrize("name", ["tree7", "rand90"])
@pytest.mark.parametrize("mutant", fk.VJP_MUTANTS)
def test_vjp_gate_rejects(name, mutant):
    c = fk.case(name)
    e = fk.vjp_error(fk.vjp(c["x"], c["g"], c["sk"], c["mean"], c["std"], F64, mutant=mutant), c)
    print(f"[fk] {name} / {mutant}: gradient {e:.3e} (gate {fk.MARGIN * c['eps']['vjp']:.3e})")
    assert c["eps"]["vjp"] > 0 and e > fk.MARGIN * c["eps"]["vjp"]


def test_yardsticks_are_float32_sized():
    for name in fk.SKELETONS[:4]:
        eps = fk.case(name)["eps"]
        print(f"[fk] {name}: eps_ref {eps}")
        assert all(0 <= v < 1e-4 for v in eps.values()), (name, eps)


# ---- Skeleton ------------------------------------------------------------------------------------------------------------------------------------
def test_skeleton_validation():
    ok = dict(parents=[-1, 0, 1], offsets=np.ones((3, 3)), channel_joint=[2, 0])
    s = glue.Skeleton(**ok)
    assert (s.joints, s.channels) == (3, 2) and s.joint_channel.tolist() == [1, -1, 0]
    assert np.array_equal(s.rest_rot, np.broadcast_to(np.eye(3), (3, 3, 3)))
    assert abs(s.bone_length - 3 * np.sqrt(3)) < 1e-12
    bad = [dict(ok, parents=[0, 0, 1]), dict(ok, parents=[-1, 1, 0]), dict(ok, parents=[-1, 0, 2]), dict(ok, parents=[-1, -1, 0]),
           dict(ok, channel_joint=[0, 0]), dict(ok, channel_joint=[3]), dict(ok, channel_joint=[-1]), dict(ok, channel_joint=[]),
           dict(ok, offsets=np.full((3, 3), np.nan)), dict(ok, offsets=np.full((3, 3), np.inf)), dict(ok, offsets=np.ones((2, 3))),
           dict(parents=[], offsets=np.zeros((0, 3)), channel_joint=[0]),
           dict(parents=[-1] + list(range(256)), offsets=np.zeros((257, 3)), channel_joint=[0]),
           dict(ok, rest=np.zeros((2, 3))), dict(ok, rest=np.full((3, 3), np.nan))]
    for kw in bad:
        with pytest.raises(ValueError):
            glue.Skeleton(**kw)
    big = glue.Skeleton([-1] + list(range(255)), np.zeros((256, 3)), [0])
    assert big.joints == 256
    # rest: Rx Ry Rz in float64, the composition of the Euler conversion
    r = glue.Skeleton(**ok, rest=[[0, 0, 0], [30.0, -50.0, 110.0], [0, 0, 90.0]])
    assert np.abs(r.rest_rot - fk.euler_deg_to_matrix64([[0, 0, 0], [30.0, -50.0, 110.0], [0, 0, 90.0]])).max() < 1e-15
    assert np.abs(r.rest_rot[2] - np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]])).max() < 1e-15


BVH = """HIERARCHY
ROOT Hips
{
    OFFSET 0.0 90.5 0.0
    CHANNELS 6 Xposition Yposition Zposition Xrotation Yrotation Zrotation
    JOINT Spine
    {
        OFFSET 0.0 10.0 1.5
        CHANNELS 3 Xrotation Yrotation Zrotation
        JOINT Head
        {
            OFFSET 0.0 25.0 0.0
            CHANNELS 3 Xrotation Yrotation Zrotation
            End Site
            {
                OFFSET 0.0 8.0 0.0
            }
        }
    }
    JOINT LeftLeg
    {
        OFFSET 9.0 -2.0 0.0
        CHANNELS 3 Xrotation Yrotation Zrotation
    }
}
MOTION
Frames: 1
Frame Time: 0.0333
0 0 0 0 0 0 0 0 0 0 0 0 0 0 0
"""


def test_from_bvh_header_reads_a_five_joint_hierarchy():
    s = glue.Skeleton.from_bvh_header(BVH)
    assert s.names == ["Hips", "Spine", "Head", "Head_end", "LeftLeg"]
    assert s.parents.tolist() == [-1, 0, 1, 2, 0]
    assert np.array_equal(s.offsets, np.array([[0, 90.5, 0], [0, 10, 1.5], [0, 25, 0], [0, 8, 0], [9, -2, 0]]))
    assert s.channel_joint.tolist() == [0, 1, 2, 4] and s.joint_channel.tolist() == [0, 1, 2, -1, 3]
    pick = glue.Skeleton.from_bvh_header(BVH, joints=["LeftLeg", "Spine"])
    assert pick.channel_joint.tolist() == [4, 1]
    assert glue.Skeleton.from_bvh_header(BVH, joints=[2]).channel_joint.tolist() == [2]
    assert glue.Skeleton.from_bvh_header(BVH.split("MOTION")[0]).parents.tolist() == [-1, 0, 1, 2, 0]        # the block alone
    for broken in (BVH.replace("OFFSET 9.0 -2.0 0.0", ""), BVH.replace("}\nMOTION", "MOTION"), "HIERARCHY\nMOTION\n",
                   BVH.replace("JOINT LeftLeg", "ROOT Other"), BVH.replace("ROOT Hips", "")):
        with pytest.raises(ValueError):
            glue.Skeleton.from_bvh_header(broken)
    with pytest.raises(ValueError):
        glue.Skeleton.from_bvh_header(BVH, joints=["Tail"])


def test_c_refusals_come_before_any_launch():
    """Every refusal of the two C calls returns -1 on the host, before a device pointer is touched: made-up non-null pointers suffice."""
    from diffsheg_amd import _lib
    L, P = _lib.lib(), 0x1000
    base = dict(x=P, ld=15, rows=4, kind=0, mean=P, std=P, J=7, Jc=5, par=P, off=P, cj=P, rr=P, jc=P, lens=None, frames=0)

    def fwd(**o):
        a = dict(base, pos=P, ldp=21, wrot=P, ldw=63)
        a.update(o)
        return L.dsh_fk_positions(None, a["x"], a["ld"], a["rows"], a["kind"], a["mean"], a["std"], a["J"], a["Jc"], a["par"], a["off"], a["cj"],
                                  a["rr"], a["jc"], a["pos"], a["ldp"], a["wrot"], a["ldw"], a["lens"], a["frames"])

    def vjp(**o):
        a = dict(base, g=P, ldg=21, dx=P, lddx=15)
        a.update(o)
        return L.dsh_fk_positions_vjp(None, a["x"], a["ld"], a["rows"], a["kind"], a["mean"], a["std"], a["J"], a["Jc"], a["par"], a["off"], a["cj"],
                                      a["rr"], a["jc"], a["g"], a["ldg"], a["dx"], a["lddx"], a["lens"], a["frames"])

    bad = [dict(x=None), dict(mean=None), dict(std=None), dict(par=None), dict(off=None), dict(cj=None), dict(rr=None), dict(jc=None),
           dict(ld=14), dict(rows=-1), dict(J=0), dict(J=257), dict(Jc=0), dict(Jc=8), dict(kind=2), dict(lens=P, frames=0), dict(lens=P, frames=3)]
    for kw in bad + [dict(pos=None), dict(ldp=20), dict(ldw=62)]:
        assert fwd(**kw) == -1 and b"dsh_fk_positions" in L.dsh_last_error(), kw
    for kw in bad + [dict(g=None), dict(dx=None), dict(ldg=20), dict(lddx=14), dict(kind=1)]:
        assert vjp(**kw) == -1 and b"dsh_fk_positions_vjp" in L.dsh_last_error(), kw
    assert fwd(rows=0) == 0 and vjp(rows=0) == 0                  # nothing to do is no refusal, and launches nothing


# ---- the host side of the public calls ---------------------------------------------------------------------------------------------------------------
def test_position_metrics_on_the_host():
    a = torch.zeros(2, 4, 3, 3)
    b = a.clone()
    b[..., 0] = 2.0                                               # every joint 2 away
    m = glue.position_metrics(a, b, pck_threshold=2.5)
    assert float(m["mpjpe"]) == 2.0 and float(m["pck"]) == 1.0
    assert float(glue.position_metrics(a, b, pck_threshold=1.5)["pck"]) == 0.0
    b[1, 2:] = float("nan")                                       # padded frames count for nothing, whatever they hold
    m = glue.position_metrics(a, b, lengths=[4, 2], pck_threshold=2.5)
    assert float(m["mpjpe"]) == 2.0 and float(m["pck"]) == 1.0
    with pytest.raises(ValueError):
        glue.position_metrics(a, b[:1], pck_threshold=1.0)
    with pytest.raises(ValueError):
        glue.position_metrics(a, b, lengths=[4], pck_threshold=1.0)
