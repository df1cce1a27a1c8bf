"""GPU tests (-m gpu) of the HuBERT encoder's bf16 precision mode (HubertEncoder(.., precision="bf16"), csrc/hubert.hip step 5).

Accuracy: the encoder's distance from the FULL-precision encoder in float64 (transformers' own output in tests/golden/hubert_small.npz at the
small configuration, hubert_ref.encode at the large widths), as maximum and as rms, against the same two statistics of
hubert_bf16_ref.encode_bf16(dt=float32), the CPU restatement of the mode with its documented rounding points:
    stat(kernel - full64) <= MARGIN x stat(encode_bf16 float32 - full64).
Both are draws from the same population of bf16 roundings (which operand rounds which way differs between any two fp32 evaluations), and
MARGIN = 3 is what bf16_gates allows between two such draws.  Nothing is fixed in advance; every test prints its figures before it asserts.
Bit identities: batch row against row alone, chunk-pass sizes, ragged against dense, the residual stream behind the positional convolution
against the fp32 encoder's, and the fp32 default against itself."""
import functools

import pytest
import torch

import hubert_bf16_ref as ref
import hubert_ref
from bf16_gates import MARGIN
from diffsheg_amd import _lib, audio
from util import golden

pytestmark = pytest.mark.gpu
SMALL, LARGE = hubert_ref.SMALL, hubert_ref.LARGE


@functools.lru_cache(maxsize=1)
def small():
    fx = golden("hubert_small.npz")
    sd = hubert_ref.make_state_dict(SMALL, int(fx["sd_seed"]))
    enc = audio.HubertEncoder(SMALL, device="cuda:0", precision="bf16").load_state_dict(sd)
    waves = {int(n): hubert_ref.make_wave(int(n), int(s)) for n, s in zip(fx["wave_lens"][:4], fx["wave_seeds"][:4])}
    return fx, sd, enc, waves


def _stats(what, out, chain32, full64):
    """(max, rms) of the kernel's and of the float32 chain's distance from the full-precision float64 encoder; printed, then asserted"""
    ek, ec = out.double() - full64, chain32.double() - full64
    k = (float(ek.abs().max()), float(ek.pow(2).mean().sqrt()))
    c = (float(ec.abs().max()), float(ec.pow(2).mean().sqrt()))
    print(f"[measure] {what}: kernel max {k[0]:.3e} rms {k[1]:.3e}; encode_bf16(float32) max {c[0]:.3e} rms {c[1]:.3e}; "
          f"ratios {k[0] / c[0]:.2f} / {k[1] / c[1]:.2f}; feature range {float(full64.max() - full64.min()):.2f}")
    assert bool(torch.isfinite(out).all())
    assert k[0] <= MARGIN * c[0], f"{what}: max error {k[0]:.3e} above {MARGIN} x {c[0]:.3e}"
    assert k[1] <= MARGIN * c[1], f"{what}: rms error {k[1]:.3e} above {MARGIN} x {c[1]:.3e}"


@pytest.mark.parametrize("n", [400, 719, 720, 16000])
def test_encoder_small_bf16_against_the_full_precision_encoder(n):
    fx, sd, enc, waves = small()
    full64 = torch.from_numpy(fx[f"out64_{n}"])
    x = waves[n][None]
    chain32 = ref.encode_bf16(sd, SMALL, x, torch.float32)[0]
    out = enc.encode(x.cuda())
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.shape == (1, hubert_ref.num_frames(SMALL, n), SMALL["hidden"])
    _stats(f"bf16 encoder small n={n}", out[0].cpu(), chain32, full64)


def test_encoder_bf16_large_widths_two_layers():
    cfg = dict(LARGE, layers=2)
    sd = hubert_ref.make_state_dict(cfg, 77)
    x = torch.stack([hubert_ref.make_wave(48400, 7), hubert_ref.make_wave(48400, 8)])
    full64 = hubert_ref.encode(sd, cfg, x.double())
    assert full64.shape == (2, 151, 1024)
    chain32 = ref.encode_bf16(sd, cfg, x, torch.float32)
    enc = audio.HubertEncoder(cfg, device="cuda:0", precision="bf16").load_state_dict(sd)
    out = enc.encode(x.cuda())
    torch.cuda.synchronize()
    out = out.cpu()
    enc.close()
    _stats("bf16 encoder large widths, 2 layers, n=48400, B=2", out, chain32, full64)


def test_bf16_batch_rows_and_pass_sizes_are_bit_identical():
    fx, sd, enc, waves = small()
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


def test_bf16_ragged_rows_are_the_dense_rows():
    fx, sd, enc, waves = small()
    lens = [16000, 400, 7000, 15999, 719]
    x = torch.full((len(lens), 16000), float("nan"))
    for b, n in enumerate(lens):
        x[b, :n] = hubert_ref.make_wave(n, 70 + b)
    x = x.cuda()
    out = enc.encode(x, lengths=lens)
    for b, n in enumerate(lens):
        m = hubert_ref.num_frames(SMALL, n)
        assert torch.equal(out[b, :m], enc.encode(x[b:b + 1, :n].contiguous())[0]), f"row {b} ({n} samples) differs from the dense call on it alone"
        assert bool((out[b, m:] == 0).all())
    assert bool(torch.isfinite(out).all())


def test_residual_stream_behind_the_positional_convolution_has_the_fp32_bits():
    fx, sd, enc, waves = small()
    f32 = audio.HubertEncoder(SMALL, device="cuda:0").load_state_dict(sd)
    x = torch.stack([hubert_ref.make_wave(16000, 60 + i) for i in range(2)]).cuda()
    M = hubert_ref.num_frames(SMALL, 16000)
    taps = [torch.full((2 * M, SMALL["hidden"]), float("nan"), device="cuda") for _ in range(2)]
    outs = []
    for e, t in zip((enc, f32), taps):
        e.debug_tap(t)
        outs.append(e.encode(x))
        e.debug_tap(None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(taps[0]).all()) and torch.equal(taps[0], taps[1])
    assert not torch.equal(outs[0], outs[1]), "the bf16 layers gave the fp32 encoder's bits: the precision was not applied"
    f32.close()


def test_fp32_default_is_unchanged_by_the_argument():
    fx, sd, enc, waves = small()
    x = torch.stack([hubert_ref.make_wave(16000, 80 + i) for i in range(2)]).cuda()
    a = audio.HubertEncoder(SMALL, device="cuda:0").load_state_dict(sd)
    b = audio.HubertEncoder(SMALL, device="cuda:0", precision="fp32").load_state_dict(sd)
    assert a.precision == b.precision == "fp32" and enc.precision == "bf16"
    assert torch.equal(a.encode(x), b.encode(x))
    a.close()
    b.close()


def test_set_precision_is_refused_after_finalize():
    fx, sd, enc, waves = small()
    L = _lib.lib()
    assert L.dsh_hubert_set_precision(enc._h, 0) == -1
    assert b"before dsh_hubert_finalize" in L.dsh_last_error()
    assert L.dsh_hubert_set_precision(enc._h, 1) == -1


def test_public_path_with_a_bf16_encoder():
    from diffsheg_amd.config import get_config
    from diffsheg_amd.synthetic import make_inputs
    from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace
    from util import gpu_model
    cfg = get_config("show")
    hub_cfg = dict(LARGE, layers=1)
    hub = audio.HubertEncoder(hub_cfg, device="cuda:0", precision="bf16").load_state_dict(hubert_ref.make_state_dict(hub_cfg, 5))
    fe = audio.AudioFrontEnd(hub)
    n = 42667
    g = torch.Generator().manual_seed(21)
    wave = 0.1 * torch.randn(n, generator=g)
    mel, feat = fe.features(wave)
    N = -(-n * 9 // 8) // 1200
    assert N == 40 and mel.shape == (N, 128) and feat.shape == (N, 1024) and feat.dtype == torch.float32 and feat.is_cuda
    assert bool(torch.isfinite(mel).all()) and bool(torch.isfinite(feat).all())
    wave2 = 0.1 * torch.randn(30000, generator=g)
    melb, featb, lengths = fe.features_batch([wave, wave2])
    N2 = -(-30000 * 9 // 8) // 1200
    assert lengths == [N, N2] and melb.shape == (2, N, 128) and featb.shape == (2, N, 1024) and featb.dtype == torch.float32
    assert bool(torch.isfinite(featb).all()) and torch.equal(featb[0], feat) and bool((featb[1, N2:] == 0).all())
    tr = DDPMTrainer(sampler_namespace(cfg, n_poses=24), gpu_model("show", "fp32"))
    pid = make_inputs(cfg, 1, frames=24, seed=3)["person_id"]
    a = tr.sample_custom_audio(wave, pid, fe, seed=9)
    b = tr.sample_arbitrary_len(mel[None], pid, {"pretrain_aud_feat": feat[None]}, seed=9)
    assert a.shape == (1, N, cfg.net_dim_pose) and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    hub.close()
