"""GPU tests (-m gpu) of csrc/metrics.hip through dsh_op_batch_metrics with a CHOSEN b_div (metrics.batch_metrics only ever passes
min(50, B)), at the edges of its three launches, gated by tests/metrics_gates.py with gates derived from the kernels' own arithmetic:
sq_sum relative n_elems x 2^-53 of the exactly rounded float64 sum, the PCK count exactly that of the reference's float32 arithmetic
(joints ON the threshold included), every diversity group relative b_div x 2^-24 of its float64 value.
The result buffer is prefilled with NaN and with a second pattern (nothing may depend on what the scratch area held), SENTINEL behind it
must come back untouched, and two runs give identical bits.  Every test prints its error / gate, or `exact`."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsheg_amd import _lib  # noqa: E402
import metrics_gates as G  # noqa: E402

DEV = "cuda:0"
H = _lib.METRICS_HEADER
GUARD = 64


def _result_words(B, T, C, b_div):
    n = int(_lib.lib().dsh_batch_metrics_result_bytes(B, T, C, b_div))
    assert n > 0 and n % 8 == 0
    return n // 8


def _launch(o, m, joint_dim, b_div, prefill=G.NAN):
    """the result words (header + groups + scratch) as a CPU float64 tensor; the guard words behind them are checked"""
    B, T, Cc = o.shape
    words = _result_words(B, T, Cc, b_div)
    assert words >= H + B // b_div + 2 * 1024
    buf = torch.full((words + GUARD,), prefill, dtype=torch.float64, device=DEV)
    buf[words:] = G.SENTINEL
    _lib.check(_lib.lib().dsh_op_batch_metrics(None, C.c_void_p(o.data_ptr()), C.c_void_p(m.data_ptr()), B, T, Cc, joint_dim, b_div,
                                               C.c_void_p(buf.data_ptr())), "dsh_op_batch_metrics")
    torch.cuda.synchronize()
    res = buf.cpu()
    assert bool((res[words:] == G.SENTINEL).all()), "words behind the result buffer were written"
    return res[:words]


def _parse(res, groups):
    i = res.view(torch.int64)
    assert int(i[4]) == groups
    return {"sq_sum": float(res[0]), "count": int(i[1]), "mse": float(res[2]), "pck": float(res[3]), "div": res[H:H + groups].numpy().copy()}


def _bits(res, groups):
    return res[:H + groups].view(torch.int64).clone()


@pytest.mark.parametrize("family", G.METRIC_FAMILIES)
@pytest.mark.parametrize("shape", G.METRIC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edge_shapes(shape, family):
    B, T, Cc, jd, b_div = shape
    o, m = G.metric_inputs(*shape, family=family)
    od, md = o.to(DEV), m.to(DEV)
    groups = B // b_div
    res = _launch(od, md, jd, b_div)
    r = _parse(res, groups)
    exact, n_elems, mse_gate = G.mse_ref(o, m)
    n_joints = n_elems // jd
    want = G.pck_emul(o.numpy(), m.numpy(), jd)
    ref_div = G.div_ref(o, b_div)
    mse_r = abs(r["sq_sum"] - exact) / exact / mse_gate
    div_r = float((np.abs(r["div"] - ref_div) / ref_div).max() / G.div_gate(b_div))
    print(f"[metrics {shape} {family}] sq_sum error / gate = {mse_r:.3f} (gate {mse_gate:.2e}), pck {r['count']} vs {want} of {n_joints}: "
          f"{'exact' if r['count'] == want else 'NOT exact'}, diversity error / gate = {div_r:.3f} (gate {G.div_gate(b_div):.2e}, {groups} groups)")
    assert abs(r["sq_sum"] - exact) <= mse_gate * exact
    assert r["mse"] == r["sq_sum"] / n_elems
    assert r["count"] == want
    assert r["pck"] == r["count"] / n_joints
    G.div_check(r["div"], ref_div, b_div)
    # nothing depends on what the buffer held, and a second run gives the same bits
    again = _launch(od, md, jd, b_div, prefill=-7.0e300)
    assert torch.equal(_bits(res, groups), _bits(again, groups)), "the results depend on the previous content of the result buffer"
    assert torch.equal(_bits(res, groups), _bits(_launch(od, md, jd, b_div), groups))


def test_b_div_above_the_limit_is_refused():
    o = torch.zeros(130, 2, 6, device=DEV)
    words = _result_words(130, 2, 6, 128)
    assert _lib.lib().dsh_batch_metrics_result_bytes(130, 2, 6, 129) > 0       # (sizing is not where the limit lives)
    buf = torch.full((words + GUARD,), 5.0, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    for bd in (131, 1, 0, 129):
        assert _lib.lib().dsh_op_batch_metrics(None, C.c_void_p(o.data_ptr()), C.c_void_p(o.data_ptr()), 130, 2, 6, 3, bd, C.c_void_p(buf.data_ptr())) == -1, bd
    assert b"limited to 128" in _lib.lib().dsh_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 5.0).all())


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("offset", [0.0, 37.25])
def test_pck_on_the_threshold(seed, offset):
    """4 096 joints ON the threshold (|d| = 0.5 to the last bit of float32): about 700 have s one float32 below 0.25, 3 100 s = 0.25, 200 one
    above; a contracted addition, a 1-ulp root or <= moves hundreds of them (test_metrics_gates_cpu.py).  The count is the emulation's."""
    o, m = G.threshold_joints(4096, seed, offset)
    want = G.pck_emul(o, m, 3)
    mutants = {k: G.pck_emul(o, m, 3, **kw) for k, kw in (("fma1", {"contract": 1}), ("fma2", {"contract": 2}), ("<=", {"le": True}), ("root+1ulp", {"sqrt_high": True}))}
    od, md = (torch.from_numpy(a).reshape(2, 32, 192).to(DEV) for a in (o, m))
    r = _parse(_launch(od, md, 3, 2), 1)
    print(f"[pck threshold seed {seed} offset {offset}] count {r['count']} vs {want} of 4096: {'exact' if r['count'] == want else 'NOT exact'} (mutants would give {mutants})")
    assert r["count"] == want and r["pck"] == want / 4096


def test_pck_on_the_threshold_per_element():
    o, m = G.threshold_scalars(4096)
    want = G.pck_emul(o, m, 1)
    od, md = (torch.from_numpy(a).reshape(2, 8, 256).to(DEV) for a in (o, m))
    r = _parse(_launch(od, md, 1, 2), 1)
    print(f"[pck threshold joint_dim 1] count {r['count']} vs {want} of 4096: {'exact' if r['count'] == want else 'NOT exact'}")
    assert r["count"] == want == int((np.abs(o) < 0.5).sum())


def test_diversity_properties():
    B, T, Cc, jd, b_div = 5, 7, 36, 3, 2
    o, m = G.metric_inputs(B, T, Cc, jd, b_div)
    # identical clips: exactly 0 in every group
    same = o[:1].expand(B, T, Cc).contiguous().to(DEV)
    r = _parse(_launch(same, m.to(DEV), jd, b_div), 2)
    print(f"[diversity identical clips] {r['div']}: {'exact' if not r['div'].any() else 'NOT exact'}")
    assert r["div"].tolist() == [0.0, 0.0]
    # a group's value depends on its own clips only: neither on the other group nor on the dropped remainder (NaN included)
    base = _launch(o.to(DEV), m.to(DEV), jd, b_div)
    o1 = o.clone()
    o1[2:4] = torch.randn(2, T, Cc, generator=torch.Generator().manual_seed(5)) * 40.0
    other = _launch(o1.to(DEV), m.to(DEV), jd, b_div)
    o2 = o.clone()
    o2[4] = G.NAN
    rem = _launch(o2.to(DEV), m.to(DEV), jd, b_div)
    o3 = o.clone()
    o3[4] = 1e30
    rem2 = _launch(o3.to(DEV), m.to(DEV), jd, b_div)
    ok = (base[H].view(torch.int64) == other[H].view(torch.int64) and other[H + 1] != base[H + 1]
          and torch.equal(base[H:H + 2].view(torch.int64), rem[H:H + 2].view(torch.int64))
          and torch.equal(base[H:H + 2].view(torch.int64), rem2[H:H + 2].view(torch.int64)))
    print(f"[diversity group 0 with group 1 / the remainder overwritten] {'exact' if ok else 'NOT exact'}")
    assert ok
    G.div_check(other[H:H + 2].numpy(), G.div_ref(o1, b_div), b_div)
