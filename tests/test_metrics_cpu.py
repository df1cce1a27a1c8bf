"""CPU tests (-m "not gpu") of the validation metrics: the Frechet distance against the reference's value in the fixture, the
load-time transform of the FGD encoder (the library's own host code, evaluated with plain matmuls) against the reference's latents,
the AverageMeter and the diversity group rule."""
import argparse
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from diffsheg_amd import _lib, metrics
from diffsheg_amd.config import get_config
from diffsheg_amd.synthetic import make_motion_pair
from diffsheg_amd.weights import (FID_VAE_LENGTH, fid_conv_frames, fid_state_dict_spec, make_synthetic_fid_state_dict)
from metrics_ref import encode_ref, packed_forward
from util import golden


@pytest.mark.parametrize("ds", ["show", "beat"])
def test_frechet_distance_matches_the_reference(ds):
    fx = golden(f"metrics_{ds}.npz")
    got = metrics.frechet_distance(fx["latents_outputs"], fx["latents_motions"])
    ref = float(fx["fgd"])
    print(f"{ds}: FGD {got:.9f} reference {ref:.9f} rel {abs(got - ref) / ref:.2e}")
    assert ref >= 0.1
    assert abs(got - ref) <= 1e-6 * ref
    # symmetric, and zero against itself, to the same 1e-6 (of the distance / of the traces it is a difference of): with 64 samples
    # of dimension 300 the covariances are singular and ~236 eigenvalues of round-off size enter through a square root
    assert abs(metrics.frechet_distance(fx["latents_motions"], fx["latents_outputs"]) - got) <= 1e-6 * ref
    trace = float(np.trace(np.cov(fx["latents_motions"].astype(np.float64), rowvar=False)))
    assert abs(metrics.frechet_distance(fx["latents_motions"], fx["latents_motions"])) <= 1e-6 * trace


def test_frechet_distance_singular_covariance_is_finite():
    g = np.random.default_rng(0)
    a, b = g.standard_normal((50, 300)), g.standard_normal((50, 300)) + 0.1      # N < D: rank-deficient covariances
    v = metrics.frechet_distance(a, b)
    assert np.isfinite(v) and v > 0


@pytest.mark.parametrize("ds", ["show", "beat"])
def test_packed_weights_reproduce_the_reference_latents(ds):
    """BatchNorm fold, [out, k * C] repack, flatten permutation and K padding — the host half of dsh_fgd_finalize, read back through
    dsh_fgd_debug_packed_layer — evaluated with plain float64 matmuls give the latents the reference's HalfEmbeddingNet gave."""
    fx = golden(f"metrics_{ds}.npz")
    cfg = get_config(ds)
    sd = make_synthetic_fid_state_dict(cfg, int(fx["fid_seed"]))
    h = metrics.create_fgd_handle(cfg.n_poses, cfg.net_dim_pose, FID_VAE_LENGTH)
    try:
        metrics.load_fgd_weights(h, sd)
        layers = metrics.packed_fgd_layers(h)
    finally:
        _lib.lib().dsh_fgd_destroy(h)
    assert len(layers) == (8 if ds == "beat" else 9)
    for W, b, K in layers:
        assert W.shape[1] % 32 == 0 and 0 <= W.shape[1] - K < 32
        assert not W[:, K:].any(), "K padding must be zero"
    assert layers[0][2] == 3 * cfg.net_dim_pose and layers[4][2] == fid_conv_frames(cfg.n_poses)[3] * FID_VAE_LENGTH
    outputs, motions = make_motion_pair(cfg, int(fx["n_latent"]), int(fx["latent_seed"]))
    for x, key in ((motions, "latents_motions"), (outputs, "latents_outputs")):
        ref = torch.from_numpy(fx[key]).double()
        got = packed_forward(layers, x, cfg.n_poses, cfg.net_dim_pose)
        err = float((got - ref).abs().max() / (ref.max() - ref.min()))
        print(f"{ds} {key}: packed-weights forward vs reference, max error / range = {err:.2e}")
        assert err <= 1e-5
    # and the independent restatement the GPU tests use at the headline shapes agrees with the reference too
    got = encode_ref(sd, motions, cfg.n_poses, FID_VAE_LENGTH)
    ref = torch.from_numpy(fx["latents_motions"])
    assert float((got - ref).abs().max() / (ref.max() - ref.min())) <= 1e-5


def test_packed_weights_any_channel_count():
    """Widths that are not a multiple of 4 (the reference builds the network for expression-only / gesture-only data too) are padded
    per tap, and 64-frame clips take the same code as 88."""
    opt = argparse.Namespace(n_poses=64, net_dim_pose=103, vae_length=32)
    sd = make_synthetic_fid_state_dict(opt, 7)
    h = metrics.create_fgd_handle(64, 103, 32)
    try:
        metrics.load_fgd_weights(h, sd)
        layers = metrics.packed_fgd_layers(h)
    finally:
        _lib.lib().dsh_fgd_destroy(h)
    assert layers[0][2] == 3 * 104 and layers[4][2] == 27 * 32
    x = torch.randn(5, 70, 103, generator=torch.Generator().manual_seed(1))
    ref = encode_ref(sd, x, 64, 32, dtype=torch.float64)
    got = packed_forward(layers, x, 64, 103)
    assert float((got - ref).abs().max() / (ref.max() - ref.min())) <= 1e-5


def test_fgd_loader_refuses_unknown_misshaped_and_missing_keys():
    cfg = get_config("beat")
    sd = make_synthetic_fid_state_dict(cfg, 1)
    L = _lib.lib()
    h = metrics.create_fgd_handle(cfg.n_poses, cfg.net_dim_pose, FID_VAE_LENGTH)
    try:
        with pytest.raises(_lib.DshError, match="unknown key"):
            metrics.load_fgd_weights(h, {"pose_encoder.net.9.weight": torch.zeros(3)})
        with pytest.raises(_lib.DshError, match="expected \\[300, 192, 3\\]"):
            metrics.load_fgd_weights(h, {"pose_encoder.net.0.0.weight": torch.zeros(300, 192, 4)})
        # decoder.*, fc_logvar.* and num_batches_tracked are accepted and ignored
        metrics.load_fgd_weights(h, {k: v for k, v in sd.items() if k != "pose_encoder.out_net.4.running_var"})
        assert L.dsh_fgd_finalize(h) == -1
        assert b"missing weight pose_encoder.out_net.4.running_var" in L.dsh_last_error()
    finally:
        L.dsh_fgd_destroy(h)
    with pytest.raises(_lib.DshError):
        metrics.create_fgd_handle(34, 192, 30)          # vae_length must be a multiple of 4
    keys = [k for k, _, _ in fid_state_dict_spec(cfg)]
    assert keys[0] == "pose_encoder.net.0.0.weight" and "decoder.net.7.bias" in keys and len(keys) == len(set(keys))


def test_average_meter_arithmetic_and_group_rule():
    m = metrics.AverageMeter("mse")
    m.update(0.5, 120)
    m.update(0.25, 7)
    assert m.count == 127 and m.sum == 0.5 * 120 + 0.25 * 7 and m.avg == m.sum / 127 and m.val == 0.25
    m.reset()
    assert m.count == 0 and m.sum == 0
    assert metrics.diversity_groups(120) == (50, 2)      # the remainder of 20 clips is dropped
    assert metrics.diversity_groups(7) == (7, 1)
    assert metrics.diversity_groups(950) == (50, 19)
    with pytest.raises(ValueError):
        metrics.diversity_groups(1)                      # the reference divides by zero there


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _meter_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        m = metrics.AverageMeter("pck")
        m.update(0.25 if rank == 0 else 0.75, 100 if rank == 0 else 300)
        m.all_reduce()
        q.put((rank, m.sum, m.count, m.avg))
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_average_meter_all_reduce_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_meter_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for _, s, c, avg in got:
        assert s == 250.0 and c == 400.0 and avg == 0.625
