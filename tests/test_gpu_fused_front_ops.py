"""The three fused kernels in front of the bf16 layers, each against an fp64 evaluation of its own expression (MI355X): the encoder_aud
tail (tl_aud_tail_kernel), the layer-0 seed (tl_joint_kernel<NF, TPB>) and audio_proj (tl_aproj_kernel), through dsh_op_tl_aud_tail /
dsh_op_tl_joint / dsh_op_tl_aproj, which build the operands with the production packers (tl_aud_pack_stream, tl_joint_pack_weight,
tl_aud_pack_audio_proj).  Gates from bf16_gates.py, every element, worst element named with tile / clip / frame.

Which test holds which term of the references (each would fail with the term removed; test_bf16_gates_cpu.py shows it on the CPU):
  PE row index row % frames ............ test_joint_matches_fp64 (every shape has several clips), test_joint_integer_operands_are_exact
  null constant on the null half only .. test_joint_matches_fp64[tight / wide], test_joint_integer_operands_are_exact
  block-2 FiLM coefficients ............ test_aud_tail_matches_fp64_chain (film holds four independent 128-vectors per clip)
  h (not x) as the last residual ....... test_aud_tail_matches_fp64_chain
  per-clip FiLM row .................... test_aud_tail_matches_fp64_chain at nb > 1 (clips end inside 32-row blocks at T = 88, 11, 34, 30)

Observed on an MI355X (each test prints its figures; profiles/fused_front_ops_gpu_tests.txt; the 69 tests of the file take 1.0 s):
  every bit-equality holds as stated: audio_proj on integer operands at all five row counts with two encoders and with either one alone,
  its 256 impulse rows; the seed on integer operands at the four widths with and without the null half, its impulse rows over all 16 nf
  columns (pad columns contribute zero); the audio tail's bf16 output is the rounded fp32 output in every element, a repeated launch and
  the rows rolled by 37 are bit-identical; no guard element was written and every refusal left its outputs untouched;
  audio tail, kernel / calibration (max / rms): (300, 88, 4) 0.64 / 1.02   (44, 11, 4) 1.31 / 1.13   (290, 34, 9) 1.06 / 1.01
        (300, 88, 1) 0.95 / 1.02   (257, 88, 3) 1.05 / 0.95   (513, 30, 6) 1.11 / 1.06 - the gate is 0.22 .. 0.32 % of the output range;
  b2 offset 0 / 20 / -100: rms error 8.0e-4 / 8.4e-4 / 1.7e-3, maximum 6.4e-3 / 6.8e-3 / 1.3e-2 (the widening allows 8e-5 / 5e-2 / 1.3);
  audio_proj, random operands: worst element at 0.96 of half an ulp + the accumulation bound;
  seed: worst element at 0.21 .. 0.41 of its gate (0.41 at 8070 rows, 16 tiles per block).
"""
import ctypes as C
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import bf16_gates as G  # noqa: E402
from diffsheg_amd import _lib  # noqa: E402

DEV = "cuda:0"
SENT32, SENT16 = 0x5A5A5A5A, 0x5A5A                # sentinel bit patterns of the guard regions (1.5e16 as fp32 / bf16)


def _p(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def _up(n, m=32):
    return (n + m - 1) // m * m


@pytest.fixture(scope="module", autouse=True)
def _module_time():
    t0 = time.time()
    yield
    print(f"\n[fused front ops] total time of this file {time.time() - t0:.1f} s")


def _sent_f32(*shape):
    return torch.full(shape, SENT32, dtype=torch.int32, device=DEV).view(torch.float32)


def _sent_bf16(*shape):
    return torch.full(shape, SENT16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _is_sent(t):
    bits = t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    return torch.equal(bits, torch.full_like(bits, SENT32 if t.dtype == torch.float32 else SENT16))


# ---- encoder_aud tail ----------------------------------------------------------------------------------------------------------------------------
AUD_W = ("Ws1", "bs1", "W1", "b1", "W2", "b2", "Ws2", "bs2", "g1", "be1", "g2", "be2", "film")
AUD_SHAPES = [(300, 88, 4), (44, 11, 4), (290, 34, 9), (300, 88, 1), (257, 88, 3), (513, 30, 6)]
_AUD_REF = {}


def _aud_ref(shape):
    """Operands, fp64 chain and gates of one shape: computed once, shared, never modified."""
    if shape not in _AUD_REF:
        t = G.aud_inputs(*shape)
        _AUD_REF[shape] = (t,) + G.aud_gates(t, *shape)
    return _AUD_REF[shape]


def _aud_call(t, Mc, T, nb, dev=None, Y=None, X2=None, ld_b=256, out=None, expect=0):
    """dsh_op_tl_aud_tail with guarded outputs: out_f [Mc + 64, 128], out_b = the right half of a [Mc + 64, 256] buffer, all sentinel."""
    d = dev or {k: t[k].to(DEV) for k in AUD_W}
    Yd = (t["Y"] if Y is None else Y).to(DEV)
    Xd = (t["X2"] if X2 is None else X2).to(DEV)
    of, ob = out or (_sent_f32(Mc + 64, 128), _sent_bf16(Mc + 64, 256))
    rc = _lib.lib().dsh_op_tl_aud_tail(None, _p(Yd), _p(Xd), *(_p(d[k]) for k in AUD_W), T, nb, Mc, _p(of), _p(ob, 256), ld_b)
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.lib().dsh_last_error())
    return of, ob


def _aud_guards(of, ob, Mc):
    assert _is_sent(of[Mc:]), "fp32 output: rows behind Mc were written"
    assert _is_sent(ob[:, :128]), "the left half of the [mel | aud_feat] buffer was written"
    assert _is_sent(ob[Mc:, 128:]), "bf16 output: rows behind Mc were written"


@pytest.mark.parametrize("shape", AUD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_aud_tail_matches_fp64_chain(shape):
    """Both outputs of the fused tail against the fp64 chain with the kernel's documented rounding points, every element under
    MARGIN x (CPU calibration) + one flip of s2; rms gates as for the fused FFN; the bf16 output is the rounded fp32 output, exactly;
    nothing outside rows < Mc x the 128 output columns is touched.  (257, 88, 3): a second block with one live row and seven waves
    without one; (513, 30, 6): three blocks; (300, 88, 1): one FiLM row for the batch, the production default."""
    Mc, T, nb = shape
    t, ref, slack, rms, cal_max, st = _aud_ref(shape)
    of, ob = _aud_call(t, Mc, T, nb)
    _aud_guards(of, ob, Mc)
    Cf, Ct = of[:Mc].cpu(), ob[:Mc, 128:].cpu()
    dk = Cf.double() - ref
    k_max, k_rms = float(dk.abs().max()), float(dk.pow(2).mean().sqrt())
    cal_rms = rms / G.MARGIN
    print(f"[bf16 gate] aud tail {shape}: kernel max {k_max:.3e} rms {k_rms:.3e}; calibration max {cal_max:.3e} rms {cal_rms:.3e}; "
          f"ratios {k_max / cal_max:.2f} / {k_rms / cal_rms:.2f}; flip_bound max {float(slack.max()) - G.MARGIN * cal_max:.2e}; "
          f"gate / output range {float(slack.max()) / float(ref.max() - ref.min()):.4f}")
    what = f"aud tail {shape}"
    G.assert_close_f32(Cf, ref, slack, what + " fp32 out", frames=T, nb=nb)
    G.assert_rounded(Ct, ref, slack, what + " bf16 out", frames=T, nb=nb)
    G.assert_rms(Cf, ref, rms, what + " fp32 out rms")
    G.assert_rms(Ct, ref, rms + G.bf16_rounding_rms(ref), what + " bf16 out rms")
    G.assert_store_is_rne(Ct, Cf, what + " bf16 store")


def test_aud_tail_is_position_independent_and_repeatable():
    """One FiLM row for the batch (nb = 1): a row's result depends on nothing but the row, so rolling the rows by 37 (other lanes, other
    waves, the other block) rolls the result bit for bit; and a second launch repeats the first bit for bit (eight waves share the
    weight ring)."""
    Mc, T = 300, 88
    t = _aud_ref((Mc, T, 1))[0]
    dev = {k: t[k].to(DEV) for k in AUD_W}
    a_f, a_b = _aud_call(t, Mc, T, 1, dev)
    r_f, r_b = _aud_call(t, Mc, T, 1, dev)
    assert torch.equal(a_f.view(torch.int32), r_f.view(torch.int32)) and torch.equal(a_b.view(torch.int16), r_b.view(torch.int16))
    s_f, s_b = _aud_call(t, Mc, T, 1, dev, Y=t["Y"].roll(37, 0), X2=t["X2"].roll(37, 0))
    _aud_guards(s_f, s_b, Mc)
    assert torch.equal(s_f[:Mc].view(torch.int32), a_f[:Mc].roll(37, 0).view(torch.int32))
    assert torch.equal(s_b[:Mc, 128:].view(torch.int16), a_b[:Mc, 128:].roll(37, 0).view(torch.int16))


def test_aud_tail_layernorm_survives_a_large_row_offset():
    """LayerNorm 2 takes var = E[y2^2] - mean^2 from fp32 accumulators (the construction of the 512-wide FFN, at D = 128): an offset on b2
    must cost no more than that arithmetic allows - the calibrated gate at the offset operands plus ln_raw_moment_slack of the fp64 y2."""
    Mc, T, nb = 300, 88, 4
    t0 = _aud_ref((Mc, T, nb))[0]
    rows = torch.arange(Mc)
    A2 = (t0["g2"] * (1 + t0["film"][:, 256:384]))[(rows // T) % nb]
    errs = {}
    for off in (0.0, 20.0, -100.0):
        t = dict(t0, b2=t0["b2"] + off)
        ref, slack, rms, cal_max, st = G.aud_gates(t, Mc, T, nb)
        wide = G.ln_raw_moment_slack(st["y2"], A2, t["Ws2"])
        of, ob = _aud_call(t, Mc, T, nb)
        Cf, Ct = of[:Mc].cpu(), ob[:Mc, 128:].cpu()
        errs[off] = float((Cf.double() - ref).pow(2).mean().sqrt())
        print(f"[aud tail, y2 offset {off:+.0f}] rms err {errs[off]:.3e} max err {float((Cf.double() - ref).abs().max()):.3e}; "
              f"calibration max {cal_max:.3e}; widening max {float(wide.max()):.3e}")
        G.assert_close_f32(Cf, ref, slack + wide, f"aud tail offset {off} fp32 out", frames=T, nb=nb)
        G.assert_rounded(Ct, ref, slack + wide, f"aud tail offset {off} bf16 out", frames=T, nb=nb)
        G.assert_rms(Cf, ref, rms + float(wide.pow(2).mean().sqrt()), f"aud tail offset {off} fp32 out rms")
    print("[aud tail, y2 offset] rms err:", {k: f"{v:.2e}" for k, v in errs.items()})


# ---- audio_proj ------------------------------------------------------------------------------------------------------------------------------------
APROJ_ROWS = (1, 31, 33, 129, 300)


def _ints(shape, g, top=2, density=0.25):
    v = torch.randint(1, top + 1, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    return (v * (torch.rand(shape, generator=g) < density)).float()


def _aproj_call(X, W, b, n_enc, Mc, expect=0, x_null=False, out0_null=False, out1_null=None):
    """dsh_op_tl_aproj; outputs with 32 guard rows.  W [n_enc, 256, 256], b [n_enc, 256]."""
    Xd, Wd, bd = X.to(DEV), W.contiguous().to(DEV), b.contiguous().to(DEV)
    o0, o1 = _sent_bf16(Mc + 32, 256), _sent_bf16(Mc + 32, 256)
    if out1_null is None:
        out1_null = n_enc == 1
    rc = _lib.lib().dsh_op_tl_aproj(None, None if x_null else _p(Xd), _p(Wd), _p(bd), n_enc, None if out0_null else _p(o0),
                                    None if out1_null else _p(o1), Mc)
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.lib().dsh_last_error())
    return o0, o1


def _assert_equal(out, ref64, what, top=256):
    assert float(ref64.abs().max()) < top, "the reference is not exactly representable: the operands of this test are wrong"
    if not torch.equal(out.cpu().double(), ref64):
        G.assert_close_f32(out.cpu().float(), ref64, 0.0, what)          # raises with the worst element's position
        raise AssertionError(what)


@pytest.fixture(scope="module")
def aproj_ints():
    g = torch.Generator().manual_seed(31)
    X, W = _ints((APROJ_ROWS[-1], 256), g), _ints((2, 256, 256), g)
    b = torch.randint(-4, 5, (2, 256), generator=g).float()
    return X.bfloat16(), W, b, [X.double() @ W[e].double().T + b[e].double() for e in (0, 1)]


@pytest.mark.parametrize("Mc", APROJ_ROWS)
@pytest.mark.parametrize("n_enc", [2, 1])
def test_aproj_integer_operands_are_exact(aproj_ints, n_enc, Mc):
    """Integer X, W and bias: every sum is an exact bf16 integer, the outputs must EQUAL the fp64 product; rows behind Mc stay untouched
    (the kernel's padding lanes store into the scratch's padding rows only).  n_enc == 1 also with the second encoder's operands alone,
    as one modality alone runs it."""
    X, W, b, ref = aproj_ints
    if n_enc == 2:
        o0, o1 = _aproj_call(X[:Mc], W, b, 2, Mc)
        for e, o in enumerate((o0, o1)):
            _assert_equal(o[:Mc], ref[e][:Mc], f"audio_proj encoder {e} of 2, Mc = {Mc}")
            assert _is_sent(o[Mc:])
    else:
        for e in (0, 1):
            o0, o1 = _aproj_call(X[:Mc], W[e:e + 1], b[e:e + 1], 1, Mc)
            _assert_equal(o0[:Mc], ref[e][:Mc], f"audio_proj encoder {e} alone, Mc = {Mc}")
            assert _is_sent(o0[Mc:]) and _is_sent(o1)


def test_aproj_impulse_rows_name_the_packed_element():
    """X = the 256 one-hot rows: row k returns W[:, k] + b exactly - a wrong element of tl_aud_pack_audio_proj shows as (row = k, col = n)."""
    g = torch.Generator().manual_seed(32)
    W = torch.randint(-100, 101, (2, 256, 256), generator=g).float()
    b = torch.randint(-8, 9, (2, 256), generator=g).float()
    o0, o1 = _aproj_call(torch.eye(256).bfloat16(), W, b, 2, 256)
    for e, o in enumerate((o0, o1)):
        _assert_equal(o[:256], W[e].double().T + b[e].double(), f"audio_proj impulse rows, encoder {e}")


def test_aproj_random_operands_within_the_accumulation_bound():
    Mc = 300
    t = G.aproj_inputs(Mc, 2)
    o0, o1 = _aproj_call(t["X"], t["W"], t["b"], 2, Mc)
    for e, o in enumerate((o0, o1)):
        used = G.assert_rounded(o[:Mc].cpu(), G.aproj_ref(t, e), G.accum_bound(t["X"], t["W"][e], 256), f"audio_proj encoder {e}")
        print(f"[bf16 gate] audio_proj encoder {e}: worst element at {used:.2f} of half an ulp + the accumulation bound")


# ---- layer-0 seed ----------------------------------------------------------------------------------------------------------------------------------
JOINT_SHAPES = [(44, 11), (300, 88), (290, 34)]
JOINT_W = (103, 112, 129, 141)          # nf 7 (9 pad columns), nf 7 (none), nf 9 (15), nf 9 (3: the BEAT gesture width)


def _row1(cfg, Mc):
    return {"none": 0, "tight": _up(Mc), "wide": _up(Mc, 256) + 32}[cfg]


def _joint_call(t, Mc, T, cfg, row1=None, expect=0, w=None, frames=None, null=()):
    """dsh_op_tl_joint on the CPU operands of joint_inputs: h_out [rows + 32 guard rows, 512]."""
    row1 = _row1(cfg, Mc) if row1 is None else row1
    rows = (max(row1, 0) if cfg != "none" else 0) + _up(Mc)
    d = {k: t[k].contiguous().to(DEV) for k in ("x", "Wj", "b", "pe", "cnull")}
    for k in null:
        d[k] = None
    out = _sent_f32(rows + 32, 512)
    rc = _lib.lib().dsh_op_tl_joint(None, _p(d["x"]), t["x"].shape[1], t["c0"], w or t["w"], _p(d["Wj"]), _p(d["b"]), _p(d["pe"]),
                                    T if frames is None else frames, _p(d["cnull"]) if cfg != "none" else None, Mc, row1, _p(out))
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.lib().dsh_last_error())
    assert _is_sent(out[rows:]), "rows behind the planes were written"
    return out, row1, rows


def _joint_check(t, Mc, T, cfg, what, exact=False):
    out, row1, rows = _joint_call(t, Mc, T, cfg)
    out = out.cpu()
    (rc, rn), (sc, sn) = G.joint_ref(t, Mc, T), G.joint_slack(t, Mc, T)
    used = []
    if cfg == "none":
        halves = [("only half", out[:Mc], rc, sc)]
    else:
        halves = [("null half", out[:Mc], rn, sn), ("conditional half", out[row1:row1 + Mc], rc, sc)]
        assert not bool(out[_up(Mc):row1].any()), "rows between the halves were written"
    for name, o, r, s in halves:
        if exact:
            _assert_equal(o, r, f"{what} {name}", top=2 ** 16)
        else:
            used.append(G.assert_close_f32(o, r, s, f"{what} {name}", frames=T, nb=Mc // T))
    return used


@pytest.mark.parametrize("cfg", ["none", "tight", "wide"])
@pytest.mark.parametrize("Mc,T", JOINT_SHAPES)
@pytest.mark.parametrize("w", JOINT_W)
def test_joint_matches_fp64(w, Mc, T, cfg):
    """h = bf16(x[:, c0 : c0 + w]) Wj^T + bias + PE[row % T] on both CFG halves (null half + cnull), read back from the hi / lo planes:
    every element within the fp32 accumulation bound + one rounding per epilogue addition + the plane split.  x is a channel slice of a
    wider row (c0 > 0, ldx > c0 + 16 nf: what lies behind the slice must not enter).  tight: row1 = round_up(Mc, 32), the smallest legal."""
    t = G.joint_inputs(w, Mc, T, ldx=w + 60, c0=17)
    used = _joint_check(t, Mc, T, cfg, f"seed w {w} Mc {Mc} T {T} {cfg}")
    print(f"[bf16 gate] seed w {w} ({Mc}, {T}) {cfg}: worst element at {max(used):.3f} of the gate")


@pytest.mark.parametrize("w", [103, 141])
def test_joint_sixteen_tiles_per_block(w):
    """ceil(Mc / 128) = 64: the instantiation that walks all 16 output tiles in one block (whole-chip token counts)."""
    Mc, T = 8070, 34
    assert (Mc + 127) // 128 >= 64 and Mc % 32
    t = G.joint_inputs(w, Mc, T, ldx=w + 60, c0=17)
    used = _joint_check(t, Mc, T, "tight", f"seed w {w} Mc {Mc} (16 tiles per block)")
    print(f"[bf16 gate] seed w {w} ({Mc}, {T}) tight: worst element at {max(used):.3f} of the gate")


def _joint_int_inputs(w, Mc, T, g, ldx=None):
    ldx = ldx or w + 60
    return {"x": _ints((Mc, ldx), g), "c0": 17, "w": w, "Wj": _ints((512, w), g), "b": torch.randint(-4, 5, (512,), generator=g).float(),
            "pe": torch.randint(-1000, 1001, (T + 1, 512), generator=g).float(), "cnull": torch.randint(-1000, 1001, (512,), generator=g).float()}


@pytest.mark.parametrize("cfg", ["none", "tight"])
@pytest.mark.parametrize("w,Mc,T", [(103, 290, 34), (141, 300, 88), (112, 44, 11), (129, 44, 11)])
def test_joint_integer_operands_are_exact(w, Mc, T, cfg):
    """Integer x, Wj, bias, PE and null constant: every sum is an integer below 2^16, which hi + lo holds exactly - both halves must EQUAL
    the fp64 value."""
    t = _joint_int_inputs(w, Mc, T, torch.Generator().manual_seed(w + Mc))
    _joint_check(t, Mc, T, cfg, f"seed integers w {w} Mc {Mc} {cfg}", exact=True)


@pytest.mark.parametrize("w", [103, 141])
def test_joint_impulse_rows_name_the_packed_element(w):
    """Row k of the buffer holds a one at column c0 + k, for all 16 nf columns of the tile: rows k < w return Wj[:, k] + bias + PE exactly
    (a wrong element of tl_joint_pack_weight shows as (row = k, col = n)), rows k >= w lie behind the channel slice and must contribute
    zero - they return bias + PE."""
    nf = (w + 15) // 16
    Mc, T, c0 = 16 * nf, 16, 17
    g = torch.Generator().manual_seed(w)
    t = _joint_int_inputs(w, Mc, T, g, ldx=c0 + 16 * nf + 7)
    t["Wj"] = torch.randint(-100, 101, (512, w), generator=g).float()
    t["x"] = torch.zeros(Mc, c0 + 16 * nf + 7)
    t["x"][torch.arange(Mc), c0 + torch.arange(Mc)] = 1.0
    out, row1, rows = _joint_call(t, Mc, T, "tight")
    ref = t["b"].double() + t["pe"].double()[torch.arange(Mc) % T]
    ref[:w] += t["Wj"].double().T
    _assert_equal(out[row1:row1 + Mc], ref, f"seed impulse rows w {w}, conditional half", top=2 ** 16)
    _assert_equal(out[:Mc], ref + t["cnull"].double(), f"seed impulse rows w {w}, null half", top=2 ** 16)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """What the three launchers refuse comes back as an error naming the launcher, and no output element is written."""
    L = _lib.lib()
    Mc, T = 44, 11
    t = G.joint_inputs(103, Mc, T, ldx=200, c0=17)
    for kw in ({"w": 50}, {"w": 150}, {"row1": 45}, {"row1": 32}, {"null": ("b",)}, {"null": ("pe",)}, {"frames": 0}):
        tw = G.joint_inputs(kw.pop("w"), Mc, T, ldx=200, c0=17) if "w" in kw else t          # nf = 4 / 10: not instantiated
        out, _, _ = _joint_call(tw, Mc, T, "tight", expect=-1, **kw)
        assert b"tl_joint" in L.dsh_last_error(), (kw, L.dsh_last_error())
        assert _is_sent(out), kw
    ta = _aud_ref((44, 11, 4))[0]
    dev = {k: ta[k].to(DEV) for k in AUD_W}
    Yd, Xd = ta["Y"].to(DEV), ta["X2"].to(DEV)
    for case in ("ld_b", "Y", "X2", "out_f", "out_b", "frames"):
        of, ob = _sent_f32(Mc + 64, 128), _sent_bf16(Mc + 64, 256)
        rc = L.dsh_op_tl_aud_tail(None, None if case == "Y" else _p(Yd), None if case == "X2" else _p(Xd), *(_p(dev[k]) for k in AUD_W),
                                  0 if case == "frames" else T, 4, Mc, None if case == "out_f" else _p(of),
                                  None if case == "out_b" else _p(ob, 256), 252 if case == "ld_b" else 256)
        torch.cuda.synchronize()
        assert rc == -1 and b"tl_aud_tail" in L.dsh_last_error(), (case, rc, L.dsh_last_error())
        assert _is_sent(of) and _is_sent(ob), case
    tp = G.aproj_inputs(33, 2)
    for kw in ({"x_null": True}, {"out0_null": True}, {"out1_null": True}):
        o0, o1 = _aproj_call(tp["X"], tp["W"], tp["b"], 2, 33, expect=-1, **kw)
        assert b"tl_aproj" in L.dsh_last_error(), (kw, L.dsh_last_error())
        assert _is_sent(o0) and _is_sent(o1), kw
