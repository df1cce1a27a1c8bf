"""Soft constraints while sampling, what can be said without a GPU: every refusal check_run() makes of a guided spec
before it sees a context, the Python-side refusals, MotionGuidance.from_keyframes against a hand-built tensor, and the gradient — the
object's callable form and the tests' own restatement — against torch.autograd.grad of the energy written out in float64."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_guidance_ref as R
from diffsheg_amd import _lib
from diffsheg_amd.glue import MotionGuidance, guidance_grad_torch
from diffsheg_amd.streaming import StreamPool
from diffsheg_amd.trainer import DDPMTrainer, sample_arbitrary_len_sharded


def _opts(resp, kind=0, steps=1000):
    return _lib.SamplerOptsC(kind, steps, resp, 3, 5, 10, 1, 0, 0, 0, 1, 0, 0, 0, 0.0)


def _count(o, spec):
    lib = _lib.lib()
    d, s = C.c_int64(-7), C.c_int64(-7)
    rc = lib.dsh_sample_count(C.byref(o), C.byref(spec), C.byref(d), C.byref(s))
    return rc, d.value, s.value, lib.dsh_last_error()


def test_check_run_refusals_of_a_guided_spec():
    bad = [(_opts(25), dict(guidance=1, invert_to=4), b"reverse loop"),
           (_opts(25), dict(guidance=1, guide_space=2), b"guidance space"),
           (_opts(25), dict(guidance=1, guide_space=-1), b"guidance space"),
           (_opts(25), dict(guidance=1, guide_scale=[1.0] * 24), b"one entry per level"),
           (_opts(25), dict(guidance=1, guide_scale=[1.0] * 1000), b"one entry per level"),
           (_opts(1, kind=1, steps=50), dict(guidance=1, guide_scale=[1.0] * 25), b"one entry per level")]
    for o, fields, frag in bad:
        rc, d, s, msg = _count(o, _lib.run_spec(**fields))
        assert rc == -1 and frag in msg, (fields, rc, msg)
        assert (d, s) == (-7, -7), "a refused count wrote its outputs"
    # the fields are not read without the switch
    assert _count(_opts(25), _lib.run_spec(guide_space=7, guide_scale=[1.0] * 3))[0] == 0


@pytest.mark.parametrize("masked", [0, 1])
def test_guidance_adds_no_draw_and_no_step(masked):
    for o, n in ((_opts(25), 25), (_opts(1, kind=1, steps=50), 50)):
        if masked and o.kind == 1:
            continue
        want = _count(o, _lib.run_spec(masked=masked))
        assert want[0] == 0
        for space in (0, 1):
            assert _count(o, _lib.run_spec(masked=masked, guidance=1, guide_space=space, guide_scale=[0.5] * n))[:3] == want[:3]
            assert _count(o, _lib.run_spec(masked=masked, guidance=1, guide_space=space))[:3] == want[:3]


def test_motion_guidance_refuses_bad_terms():
    Y, W, v = torch.zeros(2, 5, 7), torch.ones(2, 5, 7), torch.ones(7)
    MotionGuidance(Y, W, v, v, "x_t", [1.0] * 3)
    assert MotionGuidance(Y).weight.eq(1).all()                   # a target alone: weight 1 everywhere
    assert MotionGuidance(vel=v).channels == 7 and MotionGuidance().channels is None
    for kw in (dict(space="x"), dict(weight=W), dict(target=Y, weight=torch.ones(2, 5, 6)), dict(target=Y, weight=-W),
               dict(target=Y.double()), dict(target=torch.zeros(5, 7)), dict(target=Y, vel=torch.ones(6)), dict(vel=torch.ones(1, 7)),
               dict(vel=v, acc=torch.ones(8)), dict(target=[0.0]), dict(acc=v.to(torch.float16))):
        with pytest.raises(ValueError):
            MotionGuidance(**kw)
    with pytest.raises(ValueError):
        MotionGuidance(Y, W).with_terms(torch.zeros(2, 5, 6), torch.zeros(2, 5, 6))
    # the x0 form is no cond_fn(x, t): the contract carries no pred_xstart
    with pytest.raises(TypeError):
        MotionGuidance(Y, W, space="x0")(torch.zeros(2, 5, 7), torch.tensor([3, 3]))
    # a level scale looks the ORIGINAL timestep up in the run's map
    g = MotionGuidance(Y + 1, W, space="x_t", level_scale=[1.0, 0.5, 0.0], timestep_map=[0, 40, 80])
    x = torch.zeros(2, 5, 7)
    assert torch.equal(g(x, torch.tensor([40, 40])), 0.5 * g(x, torch.tensor([0, 0])))
    assert g(x, torch.tensor([80, 80])).abs().max() == 0
    with pytest.raises(ValueError):
        g(x, torch.tensor([41, 41]))
    with pytest.raises(NotImplementedError):
        g(x, torch.tensor([0, 40]))


def test_paths_without_guidance_refuse_it_loudly():
    g = MotionGuidance(vel=torch.ones(4))
    with pytest.raises(NotImplementedError, match="ragged"):
        DDPMTrainer.sample_arbitrary_len(None, torch.zeros(2, 9, 3), None, {}, lengths=[9, 5], guidance=g)
    with pytest.raises(NotImplementedError, match="sharded"):
        sample_arbitrary_len_sharded(None, None, None, None, 2, guidance=g)
    with pytest.raises(NotImplementedError, match="restyle"):
        DDPMTrainer.restyle(None, None, None, None, None, {}, level=3, guidance=g)
    with pytest.raises(NotImplementedError, match="StreamPool"):
        StreamPool._refuse({"guidance": g})
    with pytest.raises(ValueError):                               # (what it refused before, it still refuses the same way)
        StreamPool._refuse({"noise_source": 1})


def test_from_keyframes_against_a_hand_built_tensor():
    B, T, Cc = 2, 9, 12
    poses = torch.arange(2 * 5, dtype=torch.float32).view(2, 5) + 1           # 2 keyframes x (columns 1..2 and 7..9)
    g = MotionGuidance.from_keyframes(poses, [3, 7], [(1, 3), (7, 10)], [0.5, 2.0], B, T, Cc, device="cpu", space="x_t", vel=torch.ones(Cc))
    Y, W = torch.zeros(B, T, Cc), torch.zeros(B, T, Cc)
    for k, (f, w) in enumerate(((3, 0.5), (7, 2.0))):
        for j, c in enumerate((1, 2, 7, 8, 9)):
            Y[:, f, c] = poses[k, j]
            W[:, f, c] = w
    assert torch.equal(g.target, Y) and torch.equal(g.weight, W) and g.space == "x_t" and g.vel is not None
    per_row = torch.stack([poses, -poses])
    g2 = MotionGuidance.from_keyframes(per_row, [3, 7], [(1, 3), (7, 10)], 1.0, B, T, Cc, device="cpu")
    assert torch.equal(g2.target[1], -g2.target[0]) and torch.equal(g2.weight, (W > 0).float()) and g2.space == "x0"
    for bad in (dict(frames=[3, 9]), dict(frames=[3, 3]), dict(frames=[]), dict(columns=[(1, 3), (2, 5)]), dict(columns=[(0, 13)]),
                dict(weight=[1.0, 2.0, 3.0]), dict(weight=-1.0), dict(poses=torch.zeros(2, 4))):
        kw = dict(poses=poses, frames=[3, 7], columns=[(1, 3), (7, 10)], weight=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            MotionGuidance.from_keyframes(kw["poses"], kw["frames"], kw["columns"], kw["weight"], B, T, Cc, device="cpu")


def _energy(z, Y, W, lv, la, lens):
    """log p(y | z), float64, written out clip by clip"""
    total = 0.0 * z.sum()                  # (an energy without any term is still a function of z: gradient 0)
    for b in range(z.shape[0]):
        L = lens[b]
        zb = z[b, :L]
        if W is not None:
            total = total - 0.5 * (W[b, :L] * (zb - (Y[b, :L] if Y is not None else 0)) ** 2).sum()
        if lv is not None and L >= 2:
            total = total - 0.5 * (lv * (zb[1:] - zb[:-1]) ** 2).sum()
        if la is not None and L >= 3:
            total = total - 0.5 * (la * (zb[2:] - 2 * zb[1:-1] + zb[:-2]) ** 2).sum()
    return total


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 34])
@pytest.mark.parametrize("terms", ["all", "no_w", "no_vel", "no_acc", "w_only_no_y"])
def test_gradient_is_the_energys(T, terms):
    B, Cc = 3, 11
    gen = torch.Generator().manual_seed(T)
    z = torch.randn(B, T, Cc, generator=gen, dtype=torch.float64, requires_grad=True)
    Y = torch.randn(B, T, Cc, generator=gen, dtype=torch.float64)
    W = torch.rand(B, T, Cc, generator=gen, dtype=torch.float64)
    lv = torch.rand(Cc, generator=gen, dtype=torch.float64)
    la = torch.rand(Cc, generator=gen, dtype=torch.float64)
    if terms == "no_w":
        Y = W = None
    elif terms == "no_vel":
        lv = None
    elif terms == "no_acc":
        la = None
    elif terms == "w_only_no_y":
        Y = lv = la = None
    for lens in ([T] * B, [T, 1, max(1, T - 2)]):
        want, = torch.autograd.grad(_energy(z, Y, W, lv, la, lens), z, allow_unused=True)
        want = 1.7 * (want if want is not None else torch.zeros_like(z))
        assert want[1, lens[1]:].abs().max() == 0 if lens[1] < T else True
        got = guidance_grad_torch(z.detach(), Y, W, lv, la, lens, 1.7)
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
        npa = lambda t: None if t is None else t.numpy()
        ref = R.grad(z.detach().numpy(), npa(Y), npa(W), npa(lv), npa(la), lens, 1.7)
        assert float(np.abs(ref - want.numpy()).max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    # the callable form (fp32 terms, the x_t contract): lengths arrive as model_kwargs['length']
    if terms == "all":
        f32 = lambda t: t.float()
        g = MotionGuidance(f32(Y), f32(W), f32(lv), f32(la), space="x_t")
        lens = [T, 1, max(1, T - 2)]
        got = g(z.detach(), torch.tensor([7] * B), length=torch.tensor(lens), y={})
        want, = torch.autograd.grad(_energy(z, f32(Y).double(), f32(W).double(), f32(lv).double(), f32(la).double(), lens), z)
        assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
