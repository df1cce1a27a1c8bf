"""GPU tests (-m gpu) of the FGD encoder (csrc/pose_encoder.hip) through metrics.HalfEmbeddingNet at the paths the headline tests never
take: batch sizes on either side of the conv kernel switch, the staging path for a misaligned input pointer with dim % 4 == 0, buffer
reuse after the batch shrinks and reserve() regrowth.

Latents are gated on every element against metrics_ref.packed_forward in float64 (the library's own packed layers, evaluated with plain
matmuls): |latent - ref64| <= MARGIN x max |packed_forward32 - ref64|, packed_forward32 being the same function in float32 with one
accumulator per output, in both K orders, over the first 32 clips (metrics_gates.encoder_gate).  The BEAT network (34 frames, 192
channels, base 300: M of layer 0 is 32 B, so B = 64 is the first batch on the <2,1> conv kernel) and the 64-frame / 103-channel / base-32
network (input staged to 104 channels).  Every test prints kernel / calibration, or `exact`."""
import argparse
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsheg_amd import _lib, metrics  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.synthetic import make_motion_pair  # noqa: E402
from diffsheg_amd.weights import FID_VAE_LENGTH, make_synthetic_fid_state_dict  # noqa: E402
import metrics_gates as G  # noqa: E402

N_CLIPS = 70


@functools.lru_cache(maxsize=None)
def _net(which):
    """(network on the GPU, clips [70, frames, dim] on the CPU, ref64 latents of all of them, calibration, (opt, state dict))"""
    if which == "beat":
        opt = get_config("beat")
        base, seed = FID_VAE_LENGTH, 11
        x = make_motion_pair(opt, N_CLIPS, 21)[0].float()
    else:
        opt = argparse.Namespace(n_poses=64, net_dim_pose=103, vae_length=32)
        base, seed = 32, 7
        x = torch.randn(N_CLIPS, 66, 103, generator=torch.Generator().manual_seed(2))
    sd = make_synthetic_fid_state_dict(opt, seed)
    h = metrics.create_fgd_handle(opt.n_poses, opt.net_dim_pose, base)
    try:
        metrics.load_fgd_weights(h, sd)
        layers = metrics.packed_fgd_layers(h)
    finally:
        _lib.lib().dsh_fgd_destroy(h)
    ref, cal = G.encoder_gate(layers, x, opt.n_poses, opt.net_dim_pose)
    return metrics.HalfEmbeddingNet(opt, sd, device="cuda:0"), x, ref, cal, (opt, sd)


def _gate(which, lat, rows, what):
    _, _, ref, cal, _ = _net(which)
    r = float((lat.cpu().double() - ref[rows]).abs().max()) / cal
    print(f"[encoder {which} {what}] kernel / calibration = {r:.3f} (calibration {cal:.2e}, latent range {float(ref.max() - ref.min()):.2f})")
    G.assert_close_f32(lat.cpu(), ref[rows], G.MARGIN * cal, f"{which} {what}")


@pytest.mark.parametrize("B", [1, 2, 63, 64])
@pytest.mark.parametrize("which", ["beat", "small"])
def test_latents_on_either_side_of_the_kernel_switch(which, B):
    net, x, _, _, _ = _net(which)
    lat = net(x[:B].cuda())
    assert lat.shape == (B, net.vae_length)
    _gate(which, lat, slice(0, B), f"B={B}")


def test_misaligned_input_takes_the_staging_path_and_gives_the_same_bits():
    net, x, _, _, _ = _net("beat")
    xb = x[:5].cuda()
    assert net.dim % 4 == 0 and xb.data_ptr() % 16 == 0
    want = net(xb)
    buf = torch.full((xb.numel() + 8,), float("nan"), device="cuda")
    view = buf[1:1 + xb.numel()].view_as(xb)
    view.copy_(xb)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    got = net(view)
    same = torch.equal(got, want)
    print(f"[encoder beat misaligned input, staged] {'exact' if same else 'max |diff| %.3e' % float((got - want).abs().max())}")
    assert same
    _gate("beat", got, slice(0, 5), "misaligned")


@pytest.mark.parametrize("which", ["beat", "small"])
def test_buffer_reuse_and_regrowth(which):
    """B = 5, then 2 (the buffers hold rows of the larger batch behind the live ones), then 70 (reserve() frees and reallocates), then the
    first 5 again: the last result equals the first bit for bit, and every one is inside the gate.  A handle of its own: the growth must
    happen HERE, whatever ran before."""
    _, x, _, _, (opt, sd) = _net(which)
    net = metrics.HalfEmbeddingNet(opt, sd, device="cuda:0")
    try:
        xd = x.cuda()
        first = net(xd[:5])
        _gate(which, first, slice(0, 5), "B=5, fresh handle")
        _gate(which, net(xd[10:12]), slice(10, 12), "B=2 after 5")
        _gate(which, net(xd), slice(0, N_CLIPS), "B=70, regrown")
        last = net(xd[:5])
        same = torch.equal(first, last)
        print(f"[encoder {which} B = 5, 2, 70, 5] {'exact' if same else 'max |diff| %.3e' % float((first - last).abs().max())}")
        assert same
    finally:
        net.close()
