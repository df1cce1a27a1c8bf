"""GPU tests (-m gpu) of the audio front end on batches of utterances of different durations: the length-aware forms of the softmax attention,
the positional convolution, the mel spectrogram, the resampler and the time interpolation as ops, HubertEncoder.encode(.., lengths=) at the
small configuration, and the public calls AudioFrontEnd.features_batch / DDPMTrainer.sample_custom_audio([..]).

The contract is exact: row b of a padded batch, restricted to its own frames, has the BITS of the dense call on that row alone at its own
length, whatever the padding holds (it is NaN here throughout), and is 0 behind.  So the comparisons are torch.equal against the dense entry
points; where a float64 oracle is compared as well, the allowance is that of the dense op's own test (its calibration function, MARGIN)."""
import ctypes as C

import pytest
import torch

import audio_ref
import hubert_ref
from diffsheg_amd import _lib, audio
from f32_gates import MARGIN, SENTINEL, _seed, assert_close_f32
from test_gpu_audio_front import attn_calibration, attn_rows, run_attention
from test_gpu_hubert import LARGE, POS_CASES, SMALL, _cal, _report, pos_inputs, small

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32).cuda()


def padded(rows, width=None):
    """[B, width, ...] with row b = rows[b] in front and NaN behind"""
    width = width or max(r.shape[0] for r in rows)
    out = torch.full((len(rows), width) + tuple(rows[0].shape[1:]), NAN)
    for b, r in enumerate(rows):
        out[b, :r.shape[0]] = r
    return out


# ---- softmax attention --------------------------------------------------------------------------------------------------------------------
ATTN_LENS = [1, 31, 32, 33, 64, 70]          # the edges of the 32-query / 32-key tiling, and a single key


@pytest.mark.parametrize("family", ["plain", "dom_last"])
def test_softmax_attention_ragged(family):
    H, M_max, B = 2, 70, len(ATTN_LENS)
    rows = [attn_rows(family, 1, M, H, torch.Generator().manual_seed(_seed("attn-ragged", family, M)))[0] for M in ATTN_LENS]
    qkv = padded(rows, M_max).cuda()
    out = torch.full((B * M_max + 2, H * 64), SENTINEL, device="cuda")
    lens = _i32(ATTN_LENS)
    _lib.check(_lib.lib().dsh_op_softmax_attention_ragged(_stream(), qkv.data_ptr(), B, M_max, H, lens.data_ptr(), out.data_ptr()),
               "dsh_op_softmax_attention_ragged")
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[B * M_max:] == SENTINEL).all()), "rows behind the output were written"
    out = out[:B * M_max].reshape(B, M_max, H * 64)
    for b, M in enumerate(ATTN_LENS):
        alone = run_attention(rows[b][None], H)[0]
        assert torch.equal(out[b, :M], alone), f"row {b} (M = {M}) differs from the dense kernel on the row alone"
        assert bool((out[b, M:] == 0).all()), f"row {b}: frames behind M = {M} are not 0"
        ref = audio_ref.softmax_attention(rows[b][None].double(), H)
        allow = attn_calibration(family, M, rows[b][None], H, ref)
        err = float((out[b, :M].double() - ref[0]).abs().max())
        print(f"[measure] ragged softmax attention {family} M={M}: max err {err:.3e}, calibration {allow / MARGIN:.3e}, "
              f"kernel / calibration {err / max(allow / MARGIN, 1e-300):.2f}")
        assert_close_f32(out[b, :M], ref[0], allow, f"ragged softmax attention {family} M={M}", frames=M, nb=1)


# ---- positional convolution ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,groups,pk", POS_CASES)
def test_pos_conv_ragged(hidden, groups, pk):
    M_max = 66
    lens = [1, pk // 2, pk // 2 + 1, 65, M_max]
    B = len(lens)
    L = _lib.lib()
    _, w, bias = pos_inputs(hidden, groups, pk, 1, 1, "ragged-w")
    wp, bd = hubert_ref.conv_weight(w).contiguous().cuda(), bias.cuda()
    rows = [pos_inputs(hidden, groups, pk, 1, M, "ragged")[0][0] for M in lens]
    # NaN behind every row's own frames, and pk frames of NaN on both sides of the batch
    buf = torch.full((B * M_max + 2 * pk, hidden), NAN)
    buf[pk:pk + B * M_max] = padded(rows, M_max).reshape(B * M_max, hidden)
    buf = buf.cuda()
    out = torch.full((B * M_max + 2, hidden), SENTINEL, device="cuda")
    lens_dev = _i32(lens)
    _lib.check(L.dsh_op_pos_conv_ragged(_stream(), buf[pk:].data_ptr(), B, M_max, hidden, groups, pk, wp.data_ptr(), bd.data_ptr(),
                                        lens_dev.data_ptr(), out.data_ptr()), "dsh_op_pos_conv_ragged")
    torch.cuda.synchronize()
    assert bool((out[B * M_max:] == SENTINEL).all()), "rows behind the output were written"
    out = out[:B * M_max].reshape(B, M_max, hidden)
    for b, M in enumerate(lens):
        alone = torch.empty(M, hidden, device="cuda")
        _lib.check(L.dsh_op_pos_conv(_stream(), rows[b].contiguous().cuda().data_ptr(), 1, M, hidden, groups, pk, wp.data_ptr(), bd.data_ptr(),
                                     alone.data_ptr()), "dsh_op_pos_conv")
        assert torch.equal(out[b, :M], alone), f"row {b} (M = {M}) differs from the dense op on the row alone"
        assert bool((out[b, M:] == 0).all()), f"row {b}: frames behind M = {M} are not 0"


# ---- mel / resample / interpolation --------------------------------------------------------------------------------------------------------
def test_mel_ragged():
    lens = [1200, 1025 + 1200, 4799, 4800, 13337]
    mel = audio.MelSpectrogram(device="cuda:0")
    g = torch.Generator().manual_seed(_seed("mel-ragged"))
    rows = [0.3 * torch.randn(n, generator=g) + 0.1 * b for b, n in enumerate(lens)]
    out = mel(padded(rows).cuda(), lengths=lens)
    assert out.shape == (len(lens), 11, 128)
    assert [n // 1200 for n in lens] == [1, 1, 3, 4, 11]
    for b, n in enumerate(lens):
        alone = mel(rows[b].cuda())
        assert alone.shape == (n // 1200, 128)
        assert torch.equal(out[b, :n // 1200], alone), f"row {b} ({n} samples) differs from the dense call on the row alone"
        assert bool((out[b, n // 1200:] == 0).all()), f"row {b}: frames behind its own are not 0"
    with pytest.raises(ValueError):
        mel(padded(rows).cuda(), lengths=[1199] + lens[1:])
    with pytest.raises(ValueError):
        mel(padded(rows).cuda(), lengths=lens[:-1] + [13338])
    mel.close()


def test_resample_poly_ragged():
    lens = [1, 8, 9, 1000, 4097]
    g = torch.Generator().manual_seed(_seed("resample-ragged"))
    rows = [torch.randn(n, generator=g) for n in lens]
    out = audio.resample_poly(padded(rows).cuda(), 9, 8, lengths=lens)
    assert out.shape == (len(lens), audio_ref.resample_len(4097, 9, 8))
    for b, n in enumerate(lens):
        alone = audio.resample_poly(rows[b].cuda(), 9, 8)
        m = audio_ref.resample_len(n, 9, 8)
        assert alone.shape == (m,)
        assert torch.equal(out[b, :m], alone), f"row {b} ({n} samples) differs from the dense call on the row alone"
        assert bool((out[b, m:] == 0).all()), f"row {b}: samples behind its own are not 0"


@pytest.mark.parametrize("channels", [1024, 100])
def test_interp_time_ragged(channels):
    pairs = [(1, 1), (2, 1), (1, 3), (49, 18), (133, 40)]
    B, Tin, Tout = len(pairs), 133, 40
    L = _lib.lib()
    g = torch.Generator().manual_seed(_seed("interp-ragged", channels))
    rows = [torch.randn(a, channels, generator=g) for a, _ in pairs]
    x = padded(rows, Tin).cuda()
    out = torch.full((B * Tout + 2, channels), SENTINEL, device="cuda")
    lens_in, lens_out = _i32(a for a, _ in pairs), _i32(o for _, o in pairs)        # (held: two temporaries would share one allocation)
    _lib.check(L.dsh_interp_time_ragged(_stream(), x.data_ptr(), B, Tin, channels, out.data_ptr(), Tout, lens_in.data_ptr(), lens_out.data_ptr()),
               "dsh_interp_time_ragged")
    torch.cuda.synchronize()
    assert bool((out[B * Tout:] == SENTINEL).all()), "rows behind the output were written"
    out = out[:B * Tout].reshape(B, Tout, channels)
    for b, (a, o) in enumerate(pairs):
        alone = torch.empty(o, channels, device="cuda")
        _lib.check(L.dsh_interp_time(_stream(), rows[b].cuda().data_ptr(), 1, a, channels, alone.data_ptr(), o), "dsh_interp_time")
        assert torch.equal(out[b, :o], alone), f"row {b} ({a} -> {o} frames) differs from the dense call on the row alone"
        assert bool((out[b, o:] == 0).all()), f"row {b}: frames behind its own are not 0"


# ---- the encoder, small configuration -------------------------------------------------------------------------------------------------------
ENC_FRAMES = [1, 2, 31, 32, 33, 49]


def test_encoder_ragged_small():
    fx, sd, enc, waves, cal = small()
    # sample counts with those frame counts, not all at the lower edge of their frame count; the batch is wider than its longest row
    lens = [400 + 320 * (f - 1) + (0, 319, 5, 0, 160, 37)[i] for i, f in enumerate(ENC_FRAMES)]
    assert [hubert_ref.num_frames(SMALL, n) for n in lens] == ENC_FRAMES
    rows = [hubert_ref.make_wave(n, 300 + i) for i, n in enumerate(lens)]
    x = padded(rows, max(lens) + 200).cuda()
    M_max = hubert_ref.num_frames(SMALL, max(lens) + 200)
    outs = []
    for p in (1, 2, 4):
        enc.set_chunk_pass(p)
        outs.append(enc.encode(x, lengths=lens))
    assert outs[0].shape == (len(lens), M_max, SMALL["hidden"])
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[2]), "the chunk-pass size changed the result"
    out = outs[2]
    for b, f in enumerate(ENC_FRAMES):
        alone = enc.encode(rows[b][None].cuda())[0]
        assert alone.shape == (f, SMALL["hidden"])
        assert torch.equal(out[b, :f], alone), f"row {b} ({f} frames) differs from encode() on the row alone"
        assert bool((out[b, f:] == 0).all()), f"row {b}: frames behind its own are not 0"
    b = ENC_FRAMES.index(49)
    xb = rows[b][None]
    ref = hubert_ref.encode(sd, SMALL, xb.double())
    own = float(_cal(lambda r: hubert_ref.encode(sd, SMALL, xb, torch.float32, r), ref).max())
    allow = torch.tensor(MARGIN * max(cal, own))
    _report("ragged encoder small, the 49-frame row", out[b, :49].cpu(), ref[0], allow)
    assert_close_f32(out[b, :49].cpu(), ref[0], allow, "ragged encoder small, the 49-frame row", frames=49, nb=1)


def test_encoder_ragged_refusals():
    fx, sd, enc, waves, _ = small()
    L = _lib.lib()
    x = torch.zeros(2, 800, device="cuda")
    o = torch.zeros(2, 2, 128, device="cuda")
    lens = lambda *v: (C.c_int64 * len(v))(*v)
    assert L.dsh_hubert_encode_ragged(enc._h, x.data_ptr(), 2, 800, lens(800, 399), o.data_ptr()) == -1
    assert b"receptive field 400" in L.dsh_last_error() and b"row 1" in L.dsh_last_error()
    assert L.dsh_hubert_encode_ragged(enc._h, x.data_ptr(), 2, 800, lens(801, 800), o.data_ptr()) == -1
    assert b"801 samples in rows of 800" in L.dsh_last_error()
    assert L.dsh_hubert_encode_ragged(enc._h, x.data_ptr(), 2, 800, None, o.data_ptr()) == -1
    assert b"null lengths" in L.dsh_last_error()
    torch.cuda.synchronize()
    assert bool((o == 0).all())
    with pytest.raises(ValueError):
        enc.encode(x, lengths=[800, 399])
    with pytest.raises(ValueError):
        enc.encode(x, lengths=[800])


# ---- the public call --------------------------------------------------------------------------------------------------------------------------
def test_features_batch_and_sample_custom_audio_list():
    from diffsheg_amd.config import get_config
    from diffsheg_amd.synthetic import make_inputs
    from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace
    from util import gpu_model
    cfg = get_config("show")
    hub_cfg = dict(LARGE, layers=1)
    hub = audio.HubertEncoder(hub_cfg, device="cuda:0").load_state_dict(hubert_ref.make_state_dict(hub_cfg, 5))
    fe = audio.AudioFrontEnd(hub)
    g = torch.Generator().manual_seed(23)
    waves = [0.1 * torch.randn(n, generator=g) for n in (42667, 9000, 325000)]       # the last: one full clip and a remainder
    assert audio.plan_chunks([int(w.shape[0]) for w in waves]) == ([(2, 0)], [(0, 0, 42667), (1, 0, 9000), (2, 320000, 5000)])
    single = [fe.features(w) for w in waves]
    mel, feat, lengths = fe.features_batch(waves)
    assert lengths == [int(m.shape[0]) for m, _ in single] == [40, 8, 304]
    assert mel.shape == (3, 304, 128) and feat.shape == (3, 304, 1024)
    for b, (m, h) in enumerate(single):
        assert torch.equal(mel[b, :lengths[b]], m), f"mel of signal {b} differs from features() on it alone"
        assert torch.equal(feat[b, :lengths[b]], h), f"HuBERT features of signal {b} differ from features() on it alone"
        assert bool((mel[b, lengths[b]:] == 0).all()) and bool((feat[b, lengths[b]:] == 0).all())
    for b, rows in enumerate(hub.encode_long_batch(waves)):
        assert torch.equal(rows, hub.encode_long(waves[b].cuda()))
    # the remainders in passes of their own (42 667 | 9 000 | 5 000 samples at min_fill = 0.75) instead of one: the same bits
    assert audio.length_groups([42667, 9000, 5000], 0.75) == [[0], [1], [2]]
    mel_g, feat_g, lengths_g = fe.features_batch(waves, min_fill=0.75)
    assert lengths_g == lengths and torch.equal(mel_g, mel) and torch.equal(feat_g, feat)
    tr = DDPMTrainer(sampler_namespace(cfg, n_poses=24), gpu_model("show", "fp32"))
    pid = make_inputs(cfg, 3, frames=24, seed=3)["person_id"]
    got = tr.sample_custom_audio(waves, pid, fe, seed=9)
    pad = torch.nn.utils.rnn.pad_sequence
    want = tr.sample_arbitrary_len(pad([m for m, _ in single], batch_first=True), pid,
                                   {"pretrain_aud_feat": pad([h for _, h in single], batch_first=True)}, lengths=lengths, seed=9)
    assert len(got) == len(want) == 3
    for b in range(3):
        assert got[b].shape[-2] == lengths[b] and torch.equal(got[b], want[b]), f"clip {b}"
    hub.close()
