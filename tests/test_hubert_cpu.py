"""CPU tests of the HuBERT encoder's host side: the oracle tests/hubert_ref.py against transformers' own HubertModel outputs stored in
tests/golden/hubert_small.npz (which pins the oracle to the real architecture), the loader and the fp64 folds of dsh_hubert_* through the
host-only dsh_hubert_debug_packed, frame counts and the chunking rule.  No GPU is touched: nothing is uploaded before dsh_hubert_finalize."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import hubert_ref
from diffsheg_amd import _lib, audio
from f32_gates import MARGIN
from util import golden

SMALL = hubert_ref.SMALL
SHORT = (400, 719, 720, 16000)


@functools.lru_cache(maxsize=1)
def fixture():
    fx = golden("hubert_small.npz")
    sd = hubert_ref.make_state_dict(SMALL, int(fx["sd_seed"]))
    # the state dict and the waves are regenerated from their seeds: a generator that changed would show here, not as a kernel error
    assert abs(sum(float(v.double().abs().sum()) for v in sd.values()) - float(fx["sd_checksum"])) <= 1e-9 * float(fx["sd_checksum"])
    waves = {}
    for n, seed, cs in zip(fx["wave_lens"], fx["wave_seeds"], fx["wave_checksums"]):
        waves[int(n)] = hubert_ref.make_wave(int(n), int(seed))
        assert abs(float(waves[int(n)].double().abs().sum()) - float(cs)) <= 1e-9 * float(cs)
    return fx, sd, waves


@pytest.mark.parametrize("n", SHORT)
def test_oracle_matches_transformers(n):
    fx, sd, waves = fixture()
    ref64 = torch.from_numpy(fx[f"out64_{n}"])
    ours = hubert_ref.encode(sd, SMALL, waves[n][None].double())[0]
    assert ours.shape == ref64.shape == (hubert_ref.num_frames(SMALL, n), SMALL["hidden"])
    rng = float(ref64.max() - ref64.min())
    assert float((ours - ref64).abs().max()) <= 1e-10 * rng
    # transformers in float32 lies inside the calibration of the oracle's own float32 chain
    cal = max(float((hubert_ref.encode(sd, SMALL, waves[n][None], torch.float32, r)[0].double() - ref64).abs().max()) for r in (False, True))
    err32 = float((torch.from_numpy(fx[f"out32_{n}"]).double() - ref64).abs().max())
    print(f"[measure] n={n}: transformers fp32 err {err32:.3e}, oracle chain32 calibration {cal:.3e}")
    assert err32 <= MARGIN * cal


@pytest.fixture(scope="module")
def handle():
    fx, sd, _ = fixture()
    enc = audio.HubertEncoder(SMALL, device=None)
    enc.load_tensors(sd)
    yield enc, sd
    enc.close()


def test_both_weight_norm_spellings_pack_alike(handle):
    enc, sd = handle
    fx, _, _ = fixture()
    old = hubert_ref.make_state_dict(SMALL, int(fx["sd_seed"]), old_names=True)
    assert hubert_ref.POS + "weight_g" in old and hubert_ref.POS + "parametrizations.weight.original0" in sd
    enc2 = audio.HubertEncoder(SMALL, device=None)
    old["masked_spec_embed"] = torch.zeros(SMALL["hidden"])
    old["lm_head.weight"] = torch.zeros(32, SMALL["hidden"])
    enc2.load_tensors(old)
    for a, b in zip(enc.packed("pos_conv"), enc2.packed("pos_conv")):
        assert np.array_equal(a, b)
    enc2.close()


def test_loader_refusals():
    fx, sd, _ = fixture()
    L = _lib.lib()
    enc = audio.HubertEncoder(SMALL, device=None)
    one = (C.c_int64 * 1)(128)
    z = torch.zeros(128)
    assert L.dsh_hubert_load_tensor(enc._h, b"encoder.layer_norm.weight", C.c_void_p(z.data_ptr()), one, 1) == 0
    assert L.dsh_hubert_load_tensor(enc._h, b"encoder.layer_norm.gamma", C.c_void_p(z.data_ptr()), one, 1) == -1
    assert b"unknown key" in L.dsh_last_error()
    bad = (C.c_int64 * 1)(64)
    assert L.dsh_hubert_load_tensor(enc._h, b"encoder.layer_norm.bias", C.c_void_p(z.data_ptr()), bad, 1) == -1
    assert b"expected [128]" in L.dsh_last_error()
    # finalize names the first missing key (and needs no device to find it missing)
    assert L.dsh_hubert_finalize(enc._h) == -1
    assert b"missing weight feature_extractor.conv_layers.0.conv.weight" in L.dsh_last_error()
    enc.close()


@pytest.mark.parametrize("change", [dict(heads=4), dict(conv_dim=(64,) * 6 + (48,)), dict(pos_groups=8), dict(pos_kernel=15), dict(ln_eps=1e-6)])
def test_unsupported_configurations_are_refused(change):
    with pytest.raises(_lib.DshError):
        audio.HubertEncoder(dict(SMALL, **change), device=None)


def test_large_configuration_is_accepted():
    enc = audio.HubertEncoder(audio.HubertEncoder.LARGE, device=None)
    assert [enc.num_frames(n) for n in (399, 400, 719, 720, 320080)] == [-1, 1, 1, 2, 1000]
    enc.close()


@pytest.mark.parametrize("n,frames", [(399, -1), (400, 1), (719, 1), (720, 2), (320080, 1000)])
def test_frame_counts(handle, n, frames):
    assert handle[0].num_frames(n) == frames == hubert_ref.num_frames(SMALL, n)
    if n >= 400:
        assert frames == (n - 400) // 320 + 1


def test_packed_weights_equal_the_float64_folds(handle):
    enc, sd = handle
    H = SMALL["hidden"]
    # convolutions: [out, in, k] -> [out, k in], tap-major
    for i in range(7):
        W, b, c = enc.packed("conv", i)
        k = f"feature_extractor.conv_layers.{i}.conv."
        assert np.array_equal(W, hubert_ref.conv_weight(sd[k + "weight"]).numpy()) and np.array_equal(b, sd[k + "bias"].numpy()) and not c.any()
    # positional convolution: g v / |v| in float64, tap-major
    W, b, c = enc.packed("pos_conv")
    assert np.array_equal(W, hubert_ref.conv_weight(hubert_ref.pos_conv_weight(sd, torch.float64)).float().numpy())
    assert np.array_equal(b, sd[hubert_ref.POS + "bias"].numpy())
    # feature projection: its LayerNorm folded
    Wf, bf, cf = hubert_ref.fold64(sd["feature_projection.projection.weight"], sd["feature_projection.projection.bias"],
                                   sd["feature_projection.layer_norm.weight"], sd["feature_projection.layer_norm.bias"])
    for got, want in zip(enc.packed("feat_proj"), (Wf, bf, cf)):
        assert np.array_equal(got, want.numpy())
    for l in range(SMALL["layers"]):
        k = f"encoder.layers.{l}."
        Wq = torch.cat([sd[k + f"attention.{p}_proj.weight"] * s for p, s in (("q", 0.125), ("k", 1.0), ("v", 1.0))])
        bq = torch.cat([sd[k + f"attention.{p}_proj.bias"] * s for p, s in (("q", 0.125), ("k", 1.0), ("v", 1.0))])
        for got, want in zip(enc.packed("qkv", l), hubert_ref.fold64(Wq, bq, sd[k + "layer_norm.weight"], sd[k + "layer_norm.bias"])):
            assert got.shape[0] == 3 * H and np.array_equal(got, want.numpy())
        for got, want in zip(enc.packed("ffn_in", l), hubert_ref.fold64(sd[k + "feed_forward.intermediate_dense.weight"],
                                                                         sd[k + "feed_forward.intermediate_dense.bias"],
                                                                         sd[k + "final_layer_norm.weight"], sd[k + "final_layer_norm.bias"])):
            assert np.array_equal(got, want.numpy())
        for kind, key in (("out_proj", "attention.out_proj"), ("ffn_out", "feed_forward.output_dense")):
            W, b, c = enc.packed(kind, l)
            assert np.array_equal(W, sd[k + key + ".weight"].numpy()) and np.array_equal(b, sd[k + key + ".bias"].numpy()) and not c.any()


def test_fold_reproduces_layernorm_then_linear(handle):
    """rstd (x W'^T - mean c) + d == Linear(LayerNorm(x)) in float64 with the packed operands, to the fp32 rounding of W', c, d"""
    enc, sd = handle
    W, d, c = (torch.from_numpy(a).double() for a in enc.packed("qkv", 1))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(50, SMALL["hidden"], generator=g, dtype=torch.float64) * 2 + 0.5
    mean, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    got = (x @ W.T - mean * c) / torch.sqrt(var + 1e-5) + d
    k = "encoder.layers.1."
    a = torch.nn.functional.layer_norm(x, (SMALL["hidden"],), sd[k + "layer_norm.weight"].double(), sd[k + "layer_norm.bias"].double(), 1e-5)
    want = torch.cat([(a @ sd[k + f"attention.{p}_proj.weight"].double().T + sd[k + f"attention.{p}_proj.bias"].double()) * s
                      for p, s in (("q", 0.125), ("k", 1.0), ("v", 1.0))], -1)
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_chunking_on_the_long_wave():
    fx, sd, waves = fixture()
    n = 2 * 320000 + 5000
    x = waves[n].double()
    calls = []

    def enc(batch):
        calls.append(tuple(batch.shape))
        return hubert_ref.encode(sd, SMALL, batch)

    out = hubert_ref.chunked(enc, x)
    assert calls == [(2, 320080), (1, 5000)]                         # the full chunks as ONE batch, then the remainder
    assert out.shape == ((n - 80) // 320, SMALL["hidden"]) == (int(fx["long_num_rows"]), 128)
    ref = torch.from_numpy(fx["long64"])
    rows = torch.from_numpy(fx["long_rows"])
    assert float((out[rows] - ref).abs().max()) <= 1e-10 * float(ref.max() - ref.min())
    # the library's chunking is the same rule
    out2 = audio.chunked_encode(enc, x)
    assert torch.equal(out, out2)


@pytest.mark.parametrize("n", [320000 + 400, 320000 + 399, 400, 320000 + 79, 719, 720, 2 * 320000])
def test_chunking_cut_and_pad_rule(n):
    """row counts of the pieces against (n - 80) // 320: one row too many is cut, one too few is padded with zeros"""
    def enc(batch):
        M = hubert_ref.num_frames(SMALL, batch.shape[1])
        return torch.ones(batch.shape[0], M, 4)
    out = audio.chunked_encode(enc, torch.zeros(n))
    assert out.shape[0] == (n - 80) // 320
    pieces = [min(320080, n - i * 320000) for i in range(n // 320000)] + ([n - (n // 320000) * 320000] if n - (n // 320000) * 320000 >= 400 else [])
    got = sum(hubert_ref.num_frames(SMALL, p) for p in pieces)
    assert abs(got - out.shape[0]) <= 1
    assert float(out.sum()) == 4.0 * min(got, out.shape[0])            # padded rows are zeros
    assert torch.equal(out, hubert_ref.chunked(enc, torch.zeros(n)))


def test_chunking_refuses_a_wrong_row_count():
    with pytest.raises(ValueError):
        audio.chunked_encode(lambda b: torch.ones(b.shape[0], 5, 4), torch.zeros(16000))
    with pytest.raises(ValueError):
        audio.chunked_encode(lambda b: torch.ones(b.shape[0], 1, 4), torch.zeros(399))
