"""GPU tests (-m gpu) of the HuBERT encoder (csrc/hubert.hip): its new kernels as ops (positional convolution, first convolution with its
LayerNorm + GELU, a strided convolution + LayerNorm / GELU row pass), the whole encoder at the small configuration against transformers' own
output in tests/golden/hubert_small.npz, at the large widths against the CPU oracle tests/hubert_ref.py, and the public call
(AudioFrontEnd.features, DDPMTrainer.sample_custom_audio).

Gates in the project's form (bf16_gates.py / f32_gates.py): EVERY element |out - ref64| <= MARGIN x max |chain32 - ref64|, ref64 the oracle in
float64, chain32 the oracle in float32 with one accumulator per sum in both K orders, over the launch's own rows and further rows of the same
family until the population has CAL_ROWS rows; the all-constant row of the "const" family is a population of its own (f32_gates.gate).  No
tolerance is fixed in advance; every test prints kernel / calibration in front of its assertion.
"""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import hubert_ref
from diffsheg_amd import _lib, audio
from f32_gates import CAL_ROWS, MARGIN, SENTINEL, _seed, assert_close_f32
from util import golden

pytestmark = pytest.mark.gpu
SMALL, LARGE = hubert_ref.SMALL, hubert_ref.LARGE


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cal(fn32, ref):
    """max |chain32 - ref64| over both summation orders, per row [rows]"""
    return torch.maximum(*((fn32(r).double() - ref).abs().reshape(-1, ref.shape[-1]).amax(-1) for r in (False, True)))


def _report(what, out, ref, allow):
    err = (out.double() - ref).abs()
    print(f"[measure] {what}: max err {float(err.max()):.3e}, calibration {float(allow.max()) / MARGIN:.3e}, "
          f"kernel / calibration {float((err / allow.clamp_min(1e-300)).max()) * MARGIN:.2f}")


# ---- positional convolution -------------------------------------------------------------------------------------------------------------
POS_CASES = [(128, 2, 16), (1024, 16, 128)]


def pos_inputs(hidden, groups, pk, B, M, tag):
    g = torch.Generator().manual_seed(_seed("pos", hidden, groups, pk, B, M, tag))
    cg = hidden // groups
    v = torch.randn(hidden, cg, pk, generator=g)
    w = hubert_ref.pos_conv_weight({hubert_ref.POS + "weight_g": v.double().pow(2).sum((0, 1), keepdim=True).sqrt().float() * 1.3,
                                    hubert_ref.POS + "weight_v": v}, torch.float64).float() * (8.0 / (pk * cg) ** 0.5)
    return torch.randn(B, M, hidden, generator=g), w, 0.3 * torch.randn(hidden, generator=g)


@functools.lru_cache(maxsize=None)
def pos_extra_calibration(hidden, groups, pk):
    h, w, b = pos_inputs(hidden, groups, pk, 1, CAL_ROWS, "cal")
    ref = hubert_ref.pos_conv(h, w, b, groups, torch.float64)
    return float(_cal(lambda r: hubert_ref.pos_conv(h, w, b, groups, torch.float32, r), ref).max())


@pytest.mark.parametrize("hidden,groups,pk", POS_CASES)
@pytest.mark.parametrize("B,Msel", [(1, "small"), (1, "tiles"), (1, "200"), (2, "k/2+1"), (3, "65")])
def test_pos_conv(hidden, groups, pk, B, Msel):
    Ms = {"small": (1, 2, pk // 2 - 1, pk // 2, pk // 2 + 1), "tiles": (63, 64, 65), "200": (200,), "k/2+1": (pk // 2 + 1,), "65": (65,)}[Msel]
    L = _lib.lib()
    for M in Ms:
        h, w, b = pos_inputs(hidden, groups, pk, B, M, "run")
        ref = hubert_ref.pos_conv(h, w, b, groups, torch.float64)
        own = float(_cal(lambda r: hubert_ref.pos_conv(h, w, b, groups, torch.float32, r), ref).max())
        allow = torch.tensor(MARGIN * (max(own, pos_extra_calibration(hidden, groups, pk)) if B * M < CAL_ROWS else own))
        # NaN in the caller's memory on both sides of the [0, M) frames of the batch: pk frames each
        buf = torch.full((B * M + 2 * pk, hidden), float("nan"))
        buf[pk:pk + B * M] = h.reshape(B * M, hidden)
        buf = buf.cuda()
        out = torch.full((B * M + 2, hidden), SENTINEL, device="cuda")
        wp = hubert_ref.conv_weight(w).contiguous().cuda()
        _lib.check(L.dsh_op_pos_conv(_stream(), buf[pk:].data_ptr(), B, M, hidden, groups, pk, wp.data_ptr(), b.cuda().data_ptr(), out.data_ptr()),
                   "dsh_op_pos_conv")
        torch.cuda.synchronize()
        out = out.cpu()
        assert bool((out[B * M:] == SENTINEL).all()), "rows behind the output were written"
        _report(f"pos conv hidden={hidden} k={pk} B={B} M={M}", out[:B * M], ref.reshape(B * M, hidden), allow)
        assert_close_f32(out[:B * M], ref.reshape(B * M, hidden), allow, f"pos conv hidden={hidden} B={B} M={M}", frames=M, nb=B)
        if B > 1:      # a clip's neighbours in the batch count as zeros too: row b alone gives the same bits
            o1 = torch.empty(M, hidden, device="cuda")
            _lib.check(L.dsh_op_pos_conv(_stream(), h[1].contiguous().cuda().data_ptr(), 1, M, hidden, groups, pk, wp.data_ptr(),
                                         b.cuda().data_ptr(), o1.data_ptr()))
            assert torch.equal(o1.cpu(), out[M:2 * M])


# ---- convolutions with LayerNorm + GELU ---------------------------------------------------------------------------------------------------
CONV_FAMILIES = ("plain", "off+50", "lowvar", "const")
CONV_LAYERS = [("conv0", 10, 5), ("k3", 3, 2), ("k2", 2, 2)]


def conv_inputs(layer, C_, family, Lout, rows_extra=0):
    """x (channels-last [1, L, Cin], Cin = 1 for conv0), weight [C, Cin, k], bias, gamma, beta.  The families act on the LayerNorm's input, the
    convolution's output: off+50 adds 50 to every channel (bias), lowvar scales it to a spread of 3e-3, const makes one output frame all-equal
    (its input frames are zero and the bias is one value)."""
    name, k, s = layer
    cin = 1 if name == "conv0" else C_
    Lo = Lout + rows_extra
    L = (Lo - 1) * s + k
    g = torch.Generator().manual_seed(_seed("conv", name, C_, family, Lout))
    x = torch.randn(1, L, cin, generator=g)
    w = torch.randn(C_, cin, k, generator=g) * (1.0 / (cin * k)) ** 0.5
    b = 0.3 * torch.randn(C_, generator=g)
    special = []
    if family == "off+50":
        b = b + 50.0
    elif family == "lowvar":
        w, b = w * 3e-3, b * 3e-3
    elif family == "const":
        b = torch.full((C_,), 0.7)
        t = (Lout - 1) // 2
        x[0, t * s:t * s + k] = 0.0
        special = [t]
    return x, w, b, 1 + 0.3 * torch.randn(C_, generator=g), 0.3 * torch.randn(C_, generator=g), special


def const_row_mean_slack(C_, c, gamma, eps=1e-5):
    """The all-constant row needs more than MARGIN x its calibration at C = 512 (measured on an MI355X: 3.4e-5 against a calibration of 4.7e-8;
    C = 64 stays inside).  The term responsible is the rounding of the row MEAN: the kernels add the C / 64 channels of a lane one after the
    other and join the lanes by a butterfly.  With all channels equal to c the butterfly doubles equal partial sums, which is exact, so the
    sum carries the C / 64 - 1 roundings of a lane's chain, each at most 2^-24 of a partial sum <= (C / 64) |c|; divided by C the mean is off by
    at most (C / 64 - 1) 2^-24 |c|.  torch's LayerNorm happens to sum these rows exactly, so the chain does not show the term.  Every channel
    of the row is then that same delta instead of 0, the variance is delta^2 << eps, and rstd = eps^-1/2 = 316 multiplies it:
        |y - beta| <= (C / 64 - 1) 2^-24 |c| eps^-1/2 max |gamma|,   through the GELU (Lipschitz GELU_LIP = 1.13).
    At C = 64 the term is 0: a lane holds one channel."""
    from bf16_gates import GELU_LIP
    return (-(-C_ // 64) - 1) * 2.0 ** -24 * abs(c) * eps ** -0.5 * float(gamma.abs().max()) * GELU_LIP


@pytest.mark.parametrize("family", CONV_FAMILIES)
@pytest.mark.parametrize("C_", [64, 512])
@pytest.mark.parametrize("layer", CONV_LAYERS, ids=[c[0] for c in CONV_LAYERS])
def test_conv_ln_gelu(layer, C_, family):
    name, k, s = layer
    L = _lib.lib()
    for Lout in (1, 2, 63, 64, 65):
        extra = max(0, CAL_ROWS - Lout)                  # the launch gets the first Lout output frames, the calibration sees CAL_ROWS
        x, w, b, gamma, beta, special = conv_inputs(layer, C_, family, Lout, extra)
        ref = hubert_ref.conv_ln_gelu(x, w, b, gamma, beta, k, s, torch.float64)[0]
        cal = _cal(lambda r: hubert_ref.conv_ln_gelu(x, w, b, gamma, beta, k, s, torch.float32, r)[0], ref)
        rest = torch.ones(cal.shape[0], dtype=torch.bool)
        rest[special] = False
        allow = torch.full((cal.shape[0], 1), MARGIN * float(cal[rest].max()), dtype=torch.float64)
        for r in special:
            allow[r] = MARGIN * float(cal[r]) + const_row_mean_slack(C_, 0.7, gamma)
        Lin = (Lout - 1) * s + k
        xin = x[0, :Lin].contiguous().cuda()
        out = torch.full((Lout + 2, C_), SENTINEL, device="cuda")
        dev = [t.contiguous().cuda() for t in (hubert_ref.conv_weight(w), b, gamma, beta)]
        if name == "conv0":
            rc = L.dsh_op_conv0_ln_gelu(_stream(), xin.data_ptr(), 1, Lin, C_, k, s, *[t.data_ptr() for t in dev], out.data_ptr())
        else:
            rc = L.dsh_op_conv_ln_gelu(_stream(), xin.data_ptr(), 1, Lin, C_, C_, k, s, *[t.data_ptr() for t in dev], out.data_ptr())
        _lib.check(rc, "conv + LayerNorm + GELU")
        torch.cuda.synchronize()
        out = out.cpu()
        assert bool((out[Lout:] == SENTINEL).all()), "rows behind the output were written"
        _report(f"{name} C={C_} {family} Lout={Lout}", out[:Lout], ref[:Lout], allow[:Lout])
        assert_close_f32(out[:Lout], ref[:Lout], allow[:Lout].expand(Lout, C_), f"{name} C={C_} {family} Lout={Lout}", frames=Lout, nb=1)


# ---- the whole encoder, small configuration ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def small():
    fx = golden("hubert_small.npz")
    sd = hubert_ref.make_state_dict(SMALL, int(fx["sd_seed"]))
    enc = audio.HubertEncoder(SMALL, device="cuda:0").load_state_dict(sd)
    waves = {int(n): hubert_ref.make_wave(int(n), int(s)) for n, s in zip(fx["wave_lens"][:4], fx["wave_seeds"][:4])}
    # calibration population: CAL_ROWS frames of the same signal family
    wc = hubert_ref.make_wave(320 * (CAL_ROWS - 1) + 400, 999)[None]
    ref = hubert_ref.encode(sd, SMALL, wc.double())
    cal = float(_cal(lambda r: hubert_ref.encode(sd, SMALL, wc, torch.float32, r), ref).max())
    return fx, sd, enc, waves, cal


@pytest.mark.parametrize("n", [400, 719, 720, 16000])
def test_encoder_small_against_transformers(n):
    fx, sd, enc, waves, cal = small()
    ref = torch.from_numpy(fx[f"out64_{n}"])
    x = waves[n][None]
    own = float(_cal(lambda r: hubert_ref.encode(sd, SMALL, x, torch.float32, r), ref[None]).max())
    fix32 = float((torch.from_numpy(fx[f"out32_{n}"]).double() - ref).abs().max())
    allow = torch.tensor(MARGIN * max(cal, own, fix32))
    out = enc.encode(x.cuda())
    torch.cuda.synchronize()
    assert out.shape == (1, hubert_ref.num_frames(SMALL, n), SMALL["hidden"])
    out = out[0].cpu()
    _report(f"encoder small n={n} (transformers fp32 itself: {fix32:.3e})", out, ref, allow)
    assert_close_f32(out, ref, allow, f"encoder small n={n}", frames=out.shape[0], nb=1)


def test_encoder_batch_rows_and_pass_sizes_are_bit_identical():
    fx, sd, enc, waves, _ = small()
    g = torch.Generator().manual_seed(11)
    x = torch.stack([hubert_ref.make_wave(16000, 50 + i) for i in range(3)]).cuda()
    enc.set_chunk_pass(4)
    full = enc.encode(x)
    for b in range(3):
        assert torch.equal(enc.encode(x[b:b + 1])[0], full[b]), f"row {b} of B = 3 differs from the same row alone"
    enc.set_chunk_pass(1)
    one = enc.encode(x)
    enc.set_chunk_pass(2)
    two = enc.encode(x)
    enc.set_chunk_pass(4)
    assert torch.equal(one, full) and torch.equal(two, full), "the chunk-pass size changed the result"


def test_encoder_refusals():
    fx, sd, enc, waves, _ = small()
    L = _lib.lib()
    x = torch.zeros(2, 800, device="cuda")
    o = torch.zeros(2, 2, 128, device="cuda")
    assert L.dsh_hubert_encode(enc._h, x.data_ptr(), 1, 399, o.data_ptr()) == -1
    assert b"receptive field 400" in L.dsh_last_error()
    assert L.dsh_hubert_encode(enc._h, None, 1, 800, o.data_ptr()) == -1
    assert L.dsh_hubert_encode(enc._h, x.data_ptr(), 0, 800, o.data_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((o == 0).all())


# ---- the whole encoder, large widths --------------------------------------------------------------------------------------------------------
def test_encoder_large_widths_two_layers():
    """hubert-large's widths with 2 layers, seeded weights at transformers' initialisation scale, n = 48 400 (151 frames); two signals, so that the
    calibration population (the launch's own rows) has more than CAL_ROWS rows"""
    cfg = dict(LARGE, layers=2)
    sd = hubert_ref.make_state_dict(cfg, 77)
    x = torch.stack([hubert_ref.make_wave(48400, 7), hubert_ref.make_wave(48400, 8)])
    ref = hubert_ref.encode(sd, cfg, x.double())
    assert ref.shape == (2, 151, 1024)
    allow = torch.tensor(MARGIN * float(_cal(lambda r: hubert_ref.encode(sd, cfg, x, torch.float32, r), ref).max()))
    enc = audio.HubertEncoder(cfg, device="cuda:0").load_state_dict(sd)
    out = enc.encode(x.cuda())
    torch.cuda.synchronize()
    out = out.cpu()
    enc.close()
    _report("encoder large widths, 2 layers, n=48400", out, ref, allow)
    assert_close_f32(out.reshape(302, 1024), ref.reshape(302, 1024), allow, "encoder large widths", frames=151, nb=2)


# ---- the public call --------------------------------------------------------------------------------------------------------------------------
def test_features_and_sample_custom_audio():
    from diffsheg_amd.config import get_config
    from diffsheg_amd.synthetic import make_inputs
    from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace
    from util import gpu_model
    cfg = get_config("show")
    hub_cfg = dict(LARGE, layers=1)
    hub = audio.HubertEncoder(hub_cfg, device="cuda:0").load_state_dict(hubert_ref.make_state_dict(hub_cfg, 5))
    fe = audio.AudioFrontEnd(hub)
    n = 42667
    g = torch.Generator().manual_seed(21)
    wave = 0.1 * torch.randn(n, generator=g)
    mel, feat = fe.features(wave)
    N = -(-n * 9 // 8) // 1200
    assert N == 40 and mel.shape == (N, 128) and feat.shape == (N, 1024) and mel.is_cuda and feat.is_cuda
    rows = fe.hubert.encode_long(wave.cuda())
    assert rows.shape == ((n - 80) // 320, 1024) == (133, 1024)
    assert bool(torch.isfinite(mel).all()) and bool(torch.isfinite(feat).all())
    # the rows are interpolated to the mel frames with align_corners = True: the first frame is the first HuBERT row
    assert torch.equal(feat[0], rows[0])
    # mel of the resampled signal == the mel front on the resampler's output; wave18k= bypasses the resampler
    w18 = audio.resample_poly(wave.cuda(), 9, 8)
    assert torch.equal(mel, fe.mel(w18)) and torch.equal(fe.features(wave, wave18k=w18)[0], mel)
    tr = DDPMTrainer(sampler_namespace(cfg, n_poses=24), gpu_model("show", "fp32"))
    pid = make_inputs(cfg, 1, frames=24, seed=3)["person_id"]
    a = tr.sample_custom_audio(wave, pid, fe, seed=9)
    b = tr.sample_arbitrary_len(mel[None], pid, {"pretrain_aud_feat": feat[None]}, seed=9)
    assert a.shape == (1, N, cfg.net_dim_pose) and torch.equal(a, b)
    c = tr.sample_custom_audio(wave, pid, fe, seed=9, cond_scale=1.5)
    d = tr.sample_arbitrary_len(mel[None], pid, {"pretrain_aud_feat": feat[None]}, seed=9, cond_scale=1.5)
    assert torch.equal(c, d)
    hub.close()
