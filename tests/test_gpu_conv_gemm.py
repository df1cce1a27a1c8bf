"""GPU tests (-m gpu) of ONE launch of the FGD encoder's implicit-GEMM Conv1d (csrc/pose_encoder.hip conv_gemm_f32_kernel) through the test
helper dsh_op_conv_gemm_f32, gated on every element by tests/metrics_gates.py: |out - ref64| <= MARGIN x max |chain32 - ref64| (no
tolerance fixed in advance; the `ints` family bit for bit), at the smallest shapes that reach each path of the launcher and the kernel —
both instantiations, the XCD block order, padded grid blocks, the row and column tails, the Kreal mask boundary, strides, clip gaps.

Every launch writes into a buffer filled with SENTINEL: the y_clip - Tout N floats behind each clip's rows and the rows behind the last clip
must come back untouched.  X holds NaN in every float that no output's Kreal window covers (the K pad behind a clip's last row, the gap
between clips, frames a stride-2 conv skips, the tail behind the last clip): one read outside a window turns outputs into NaN.
Every test prints kernel / calibration (or `exact`) in front of its assertion."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsheg_amd import _lib  # noqa: E402
import metrics_gates as G  # noqa: E402

DEV = "cuda:0"


def _p(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def _operands(t):
    return {"X": G.conv_x_flat(t).to(DEV), "W": G.conv_w_padded(t).to(DEV), "b": t["b"].to(DEV),
            "Y": torch.full((t["B"] * t["y_clip"] + G.Y_TAIL_ROWS * t["N"],), G.SENTINEL, device=DEV)}


def _call(t, o, **over):
    a = dict(X=_p(o["X"]), x_clip=t["x_clip"], x_step=t["x_step"], W=_p(o["W"]), ldw=t["ldw"], bias=_p(o["b"]), Y=_p(o["Y"]), y_clip=t["y_clip"],
             B=t["B"], Tout=t["Tout"], N=t["N"], Kreal=t["Kreal"], Kp=t["Kp"], leaky=t["leaky"])
    a.update(over)
    return _lib.lib().dsh_op_conv_gemm_f32(None, a["X"], a["x_clip"], a["x_step"], a["W"], a["ldw"], a["bias"], a["Y"], a["y_clip"], a["B"], a["Tout"],
                                           a["N"], a["Kreal"], a["Kp"], a["leaky"])


def _output(t, Y, B=None, Tout=None):
    """[B Tout, N] rows of the launch; asserts that everything else in Y still holds SENTINEL"""
    B, Tout = B or t["B"], Tout or t["Tout"]
    Yc = Y.cpu()
    body = Yc[:B * t["y_clip"]].view(B, t["y_clip"])
    assert bool((body[:, Tout * t["N"]:] == G.SENTINEL).all()), "the floats behind a clip's rows were written"
    assert bool((Yc[B * t["y_clip"]:] == G.SENTINEL).all()), "rows behind the last clip were written"
    return body[:, :Tout * t["N"]].reshape(B * Tout, t["N"])


def _run(name):
    t = G.conv_case(name)
    o = _operands(t)
    _lib.check(_call(t, o), "dsh_op_conv_gemm_f32")
    torch.cuda.synchronize()
    return t, o


@pytest.mark.parametrize("name", list(G.CONV_CASES))
def test_conv_launch_is_inside_the_derived_gate(name):
    t, o = _run(name)
    out = _output(t, o["Y"])
    print(f"[conv {name}: B {t['B']} Tout {t['Tout']} N {t['N']} Kreal {t['Kreal']} {t['family']}] kernel / calibration = {G.conv_ratio(t, out)}")
    G.conv_check(t, out, name)


def test_both_instantiations_give_the_same_bits():
    """Every output is ONE accumulator with the same K order in <1,1> and <2,1> (by reading): the first 64 rows of the M = 2049 launch
    (<2,1>, 128-row tiles, XCD order, padded grid) equal the same rows launched alone (<1,1>, one 64-row tile) bit for bit."""
    t, o = _run("dispatch-M2049")
    big = _output(t, o["Y"])[:64]
    o["Y"].fill_(G.SENTINEL)
    _lib.check(_call(t, o, B=1, Tout=64), "dsh_op_conv_gemm_f32")
    torch.cuda.synchronize()
    small = _output(t, o["Y"], B=1, Tout=64)
    same = torch.equal(big, small)
    print(f"[conv <2,1> vs <1,1>, 64 rows x {t['N']}] {'exact' if same else 'max |diff| %.3e' % float((big - small).abs().max())}")
    assert same


def test_refusals_launch_nothing():
    t = G.conv_case("width-N68-K36")
    o = _operands(t)
    assert t["Kreal"] == 36 and t["Kp"] == 64
    bad = [dict(B=0), dict(Tout=0), dict(N=0), dict(Kreal=0), dict(B=-1), dict(Tout=-3),                    # dims
           dict(Kp=48), dict(Kp=32), dict(ldw=32), dict(ldw=t["Kp"] + 2),                                   # weight padding
           dict(Kreal=34), dict(x_step=t["x_step"] + 2), dict(x_clip=t["x_clip"] + 2),                      # activation rows
           dict(N=66), dict(y_clip=t["y_clip"] + 2),                                                        # output rows
           dict(X=_p(o["X"], 4)), dict(W=_p(o["W"], 8)), dict(Y=_p(o["Y"], 4)), dict(bias=_p(o["b"], 4)),   # alignment
           dict(X=None), dict(W=None), dict(bias=None), dict(Y=None)]                                       # null pointers
    torch.cuda.synchronize()
    _lib.launch_counts(reset=True)
    for over in bad:
        assert _call(t, o, **over) == -1, over
        assert _lib.lib().dsh_last_error(), over
    assert set(_lib.launch_counts().values()) == {0}
    torch.cuda.synchronize()
    assert bool((o["Y"] == G.SENTINEL).all())
    # and the very same operands are accepted
    assert _call(t, o) == 0
    torch.cuda.synchronize()
    G.conv_check(t, _output(t, o["Y"]))
