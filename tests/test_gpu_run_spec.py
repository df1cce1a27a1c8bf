"""dsh_sample_run on a real MI355X: one call with everything in its dsh_run_spec against the same run made through the six sticky setters
and dsh_sample / dsh_invert_from, bit for bit, and what neither a completed nor a refused per-call entry may do: leave anything behind in
the context.  Synthetic "show" weights, B = 2 full windows, an 8-level log-SNR subset, Philox noise with row keys."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import fewstep_ref as F  # noqa: E402
from diffsheg_amd import _lib  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.model import UniDiffuser  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from util import synthetic_sd  # noqa: E402

DEV = "cuda:0"
KEPT, KEYS, SEEDS, SEED, START = F.LOGSNR8, [71, 72], [900, 2 ** 40 + 1], 4242, 6
B = 2


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _opts(resp, eta=0.0):
    cfg = get_config("show")
    return _lib.SamplerOptsC(0, 1000, resp, 3, 5, cfg.overlap_len, 1, 0, 0, 0, 1, SEED, 0, 0, eta)


def _u64(v):
    return (C.c_uint64 * len(v))(*v)


class _Pair:
    """Two contexts under one condition.  `spec` only ever sees dsh_sample_run (and, in the last test, setters whose values it must
    ignore); `setters` gives the raw dsh_sample of a freshly created context first, then serves the sticky-setter path."""

    def __init__(self):
        cfg = self.cfg = get_config("show")
        self.shape = (B, cfg.n_poses, cfg.net_dim_pose)
        inp = make_inputs(cfg, B, frames=cfg.n_poses, seed=3)
        self.spec, self.setters = (UniDiffuser(cfg, synthetic_sd("show"), device=DEV, precision="fp32") for _ in range(2))
        for m in (self.spec, self.setters):
            m.set_condition(inp["audio_emb"], inp["person_id"], inp["pretrain_aud_feat"])
        self.x0 = torch.randn(self.shape, generator=torch.Generator().manual_seed(8)).to(DEV)
        self.fresh = self.raw(self.setters)

    def raw(self, model):
        """dsh_sample with default options (the ddim25 stride from x_T, one Philox stream) on whatever the context holds"""
        x = torch.empty(self.shape, device=DEV)
        o = _opts(25)
        torch.cuda.synchronize()
        _lib.check(_lib.lib().dsh_sample(model._h, C.byref(o), _p(x), 0, None, None, 0, None, 0, None), "dsh_sample")
        torch.cuda.synchronize()
        return x

    def run(self, model, o, **fields):
        """(rc, x) of one dsh_sample_run from a copy of x0"""
        x = self.x0.clone()
        spec = _lib.run_spec(x=x.data_ptr(), **fields)
        torch.cuda.synchronize()
        rc = _lib.lib().dsh_sample_run(model._h, C.byref(o), C.byref(spec))
        torch.cuda.synchronize()
        return rc, x

    def close(self):
        self.spec.close()
        self.setters.close()


@pytest.fixture(scope="module")
def pair():
    p = _Pair()
    yield p
    p.close()


FULL = dict(timesteps=KEPT, solver=1, row_keys=KEYS, row_seeds=SEEDS, start_level=START, init=2)


def test_one_call_equals_the_setter_path_and_leaves_nothing_behind(pair):
    lib, h = _lib.lib(), pair.setters._h
    o = _opts(len(KEPT))
    rc, got = pair.run(pair.spec, o, **FULL)
    assert rc == 0, lib.dsh_last_error()
    assert torch.isfinite(got).all() and not torch.equal(got, pair.x0)
    # the same run through the six setters and dsh_sample
    want = pair.x0.clone()
    try:
        _lib.check(lib.dsh_sample_set_row_keys(h, _u64(KEYS), B))
        _lib.check(lib.dsh_sample_set_row_seeds(h, _u64(SEEDS), B))
        _lib.check(lib.dsh_sample_set_tail_blend(h, 0))
        _lib.check(lib.dsh_sample_set_start_level(h, START))
        _lib.check(lib.dsh_sample_set_timesteps(h, (C.c_int32 * len(KEPT))(*KEPT), len(KEPT)))
        _lib.check(lib.dsh_sample_set_solver(h, 1))
        _lib.check(lib.dsh_sample(h, C.byref(o), _p(want), 2, None, None, 0, None, 0, None), "dsh_sample")
        torch.cuda.synchronize()
        assert torch.equal(got, want), int((got != want).sum())
        # every field of the spec took part: the run without it differs
        for drop in ("solver", "row_seeds", "start_level"):
            rc, other = pair.run(pair.spec, o, **{k: v for k, v in FULL.items() if k != drop})
            assert rc == 0 and not torch.equal(other, got), drop
        # the setters ARE sticky: the raw call on their context is no longer the fresh one (its respacing of 25 now meets a list of 8)
        x = torch.empty(pair.shape, device=DEV)
        o25 = _opts(25)
        assert lib.dsh_sample(h, C.byref(o25), _p(x), 0, None, None, 0, None, 0, None) == -1 and b"respacing" in lib.dsh_last_error()
    finally:
        lib.dsh_sample_set_row_keys(h, _u64([0]), 0)
        lib.dsh_sample_set_start_level(h, 0)
        lib.dsh_sample_set_timesteps(h, (C.c_int32 * 1)(0), 0)
        lib.dsh_sample_set_solver(h, 0)
    # the per-call entry left nothing behind: the raw call on its context is the raw call on a freshly created one
    assert torch.equal(pair.raw(pair.spec), pair.fresh)
    assert torch.equal(pair.raw(pair.setters), pair.fresh)          # (and so is the setters' context once they are taken back)


def test_a_refused_call_leaves_nothing_behind(pair):
    lib = _lib.lib()
    rc, x = pair.run(pair.spec, _opts(len(KEPT), eta=0.5), **FULL)
    assert rc == -1 and b"eta" in lib.dsh_last_error()
    assert torch.equal(x, pair.x0), "a refused run wrote its sample"
    assert torch.equal(pair.raw(pair.spec), pair.fresh)
    # row keys for another batch size: refused by the run, with the setters' message
    rc, x = pair.run(pair.spec, _opts(len(KEPT)), **dict(FULL, row_keys=KEYS + [73], row_seeds=SEEDS + [5]))
    assert rc == -1 and b"row key" in lib.dsh_last_error() and torch.equal(x, pair.x0)
    assert torch.equal(pair.raw(pair.spec), pair.fresh)


def test_reverse_loops_match_and_ignore_sticky_state(pair):
    lib, h = _lib.lib(), pair.setters._h
    o = _opts(len(KEPT))
    rc, got = pair.run(pair.spec, o, timesteps=KEPT, invert_to=4)
    assert rc == 0, lib.dsh_last_error()
    want = pair.x0.clone()
    try:
        _lib.check(lib.dsh_sample_set_timesteps(h, (C.c_int32 * len(KEPT))(*KEPT), len(KEPT)))
        _lib.check(lib.dsh_invert_from(h, C.byref(o), _p(want), 0, 4, None), "dsh_invert_from")
        torch.cuda.synchronize()
    finally:
        lib.dsh_sample_set_timesteps(h, (C.c_int32 * 1)(0), 0)
    assert torch.equal(got, want) and not torch.equal(got, pair.x0)
    # two halves are the whole
    rc, half = pair.run(pair.spec, o, timesteps=KEPT, invert_to=2)
    x = half.clone()
    spec = _lib.run_spec(x=x.data_ptr(), timesteps=KEPT, invert_from=2, invert_to=4)
    assert rc == 0 and lib.dsh_sample_run(pair.spec._h, C.byref(o), C.byref(spec)) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, got)
    # sticky values an earlier setter call left in the context: the compatibility entry refuses them, the spec path does not see them
    hs = pair.spec._h
    try:
        for setter, value in ((lib.dsh_sample_set_tail_blend, 1), (lib.dsh_sample_set_start_level, 3)):
            _lib.check(setter(hs, value))
            x = pair.x0.clone()
            assert lib.dsh_invert_from(hs, C.byref(_opts(25)), _p(x), 0, 4, None) == -1
            rc, again = pair.run(pair.spec, o, timesteps=KEPT, invert_to=4)
            assert rc == 0 and torch.equal(again, got), setter.__name__
            _lib.check(setter(hs, 0))
    finally:
        lib.dsh_sample_set_tail_blend(hs, 0)
        lib.dsh_sample_set_start_level(hs, 0)
    assert torch.equal(pair.raw(pair.spec), pair.fresh)
