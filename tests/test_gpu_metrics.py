"""GPU tests (-m gpu) of the validation metrics on the device: the FGD pose encoder (csrc/pose_encoder.hip) against the reference's latents
in tests/golden/metrics_{show,beat}.npz, MSE / PCK / diversity (csrc/metrics.hip) against the reference's values there, the headline
shapes against independent torch restatements (tests/metrics_ref.py), the properties the C ABI promises, and the trainer's
validate_batch / validation_summary against a composition by hand.

Gates.  Latents: 1e-3 of the latent range, the project's fp32 bar (measured: see DESIGN.md §2).  FGD from the GPU latents against the
reference's FGD: 3 x the measured relative error, never looser than 1e-3 (FGD_GATE below; DESIGN.md §2 holds the measurement).  MSE:
relative 1e-5 — numpy's pairwise fp32 mean over 2.4 M .. 19 M terms is good to ~log2(N) 2^-24 ~ 1.5e-6 and the kernel accumulates in
fp64.  PCK: the count, exactly.  Diversity: relative 1e-4 — the reference adds 1 225 fp32 pair means sequentially, worst case
1 225 x 2^-24 ~ 7e-5; the kernel is the more exact side."""
import ctypes as C

import numpy as np
import pytest
import torch

from diffsheg_amd import _lib, metrics
from diffsheg_amd.config import get_config
from diffsheg_amd.synthetic import make_inputs, make_motion_pair
from diffsheg_amd.weights import FID_VAE_LENGTH, make_synthetic_fid_state_dict
from metrics_ref import batch_metrics_f64, encode_ref
from util import golden, gpu_model

pytestmark = pytest.mark.gpu

# relative error of FGD(GPU latents) against the reference's FGD in the fixture: measured 2.65e-7 (SHOW) / 1.22e-7 (BEAT) on an MI355X
# (of which 1.4e-7 / 7.9e-8 is frechet_distance against the reference's scipy sqrtm on identical latents, measured on the CPU):
# 3 x the larger measurement
FGD_GATE = 8.0e-7
assert FGD_GATE <= 1e-3

_NETS = {}


def fid_net(ds: str):
    if ds not in _NETS:
        cfg = get_config(ds)
        sd = make_synthetic_fid_state_dict(cfg, int(golden(f"metrics_{ds}.npz")["fid_seed"]))
        _NETS[ds] = (metrics.HalfEmbeddingNet(cfg, sd, device="cuda:0"), sd)
    return _NETS[ds]


def _range_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.max() - ref.min()))


@pytest.mark.parametrize("ds", ["show", "beat"])
def test_encoder_latents_and_fgd_match_the_reference(ds):
    fx = golden(f"metrics_{ds}.npz")
    cfg = get_config(ds)
    net, _ = fid_net(ds)
    outputs, motions = make_motion_pair(cfg, int(fx["n_latent"]), int(fx["latent_seed"]))
    lat = {}
    for x, key in ((motions, "latents_motions"), (outputs, "latents_outputs")):
        lat[key] = net(x.cuda())
        assert lat[key].shape == (int(fx["n_latent"]), FID_VAE_LENGTH) and lat[key].dtype == torch.float32
        err = _range_err(lat[key], torch.from_numpy(fx[key]))
        print(f"[measure] {ds} {key}: encoder max error / latent range = {err:.3e}")
        assert err <= 1e-3
    got = metrics.frechet_distance(lat["latents_outputs"].cpu().numpy(), lat["latents_motions"].cpu().numpy())
    ref = float(fx["fgd"])
    rel = abs(got - ref) / ref
    print(f"[measure] {ds}: FGD from GPU latents {got:.9f}, reference {ref:.9f}, relative error {rel:.3e} (gate {FGD_GATE:.1e})")
    assert rel <= FGD_GATE


@pytest.mark.parametrize("ds", ["show", "beat"])
@pytest.mark.parametrize("case", [0, 1])
def test_batch_metrics_match_the_reference(ds, case):
    fx = golden(f"metrics_{ds}.npz")
    cfg = get_config(ds)
    B, seed, jd = int(fx[f"case{case}_batch"]), int(fx[f"case{case}_seed"]), int(fx["joint_dim"])
    outputs, motions = make_motion_pair(cfg, B, seed)
    r = metrics.batch_metrics(outputs.cuda(), motions.cuda(), jd)
    torch.cuda.synchronize()
    mse, count, div = float(r["mse"]), int(r["pck_count"]), r["diversity"].cpu().numpy()
    ref_mse, ref_count, ref_div = float(fx[f"case{case}_mse"]), int(fx[f"case{case}_pck_count"]), fx[f"case{case}_diversity"]
    total = int(fx[f"case{case}_pck_total"])
    print(f"[measure] {ds} B={B}: mse rel {abs(mse - ref_mse) / ref_mse:.2e}, pck {count} vs {ref_count} of {total}, "
          f"diversity rel {np.abs(div / ref_div - 1).max():.2e}")
    assert abs(mse - ref_mse) <= 1e-5 * ref_mse
    assert count == ref_count
    assert float(r["pck"]) == count / total
    assert r["b_div"] == int(fx[f"case{case}_b_div"]) and div.shape == ref_div.shape == ((2,) if B == 120 else (1,))
    assert np.abs(div - ref_div).max() <= 1e-4 * ref_div.min()
    assert abs(float(r["sq_sum"]) / (total * jd) - mse) <= 1e-12


# (seed of the BEAT batch: the first from 1156 upwards with no joint within 1e-6 of the PCK threshold, found on the CPU: 1161)
@pytest.mark.parametrize("ds,B,seed", [("show", 950, 1850), ("beat", 256, 1161)])
def test_headline_shapes(ds, B, seed):
    """The validation batch of the reference (950 SHOW clips, 256 BEAT): metrics against float64 torch on the device, the encoder
    against the fp32 torch restatement on clips spread over the batch, first and last row included."""
    cfg = get_config(ds)
    jd = 1 if ds == "show" else 3
    outputs, motions = make_motion_pair(cfg, B, seed)
    o, m = outputs.cuda(), motions.cuda()
    r = metrics.batch_metrics(o, m, jd)
    b_div, groups = metrics.diversity_groups(B)
    ref = batch_metrics_f64(o, m, jd, b_div)
    mse, count, div = float(r["mse"]), int(r["pck_count"]), r["diversity"].cpu().numpy()
    print(f"[measure] {ds} B={B}: mse rel {abs(mse - ref['mse']) / ref['mse']:.2e}, pck {count} vs {ref['pck_count']} of {ref['pck_total']} "
          f"(margin {ref['pck_margin']:.1e}), diversity rel {np.abs(div / ref['diversity'] - 1).max():.2e}, groups {groups}")
    if jd == 3:
        assert ref["pck_margin"] >= 1e-6, "a joint lies within 1e-6 of the PCK threshold: pick another seed"
    assert abs(mse - ref["mse"]) <= 1e-5 * ref["mse"]
    assert count == ref["pck_count"]
    assert div.shape == (groups,) and np.abs(div - ref["diversity"]).max() <= 1e-4 * ref["diversity"].min()
    net, sd = fid_net(ds)
    lat = net(o)
    rows = sorted(set(np.linspace(0, B - 1, 10).astype(int).tolist()))
    assert rows[0] == 0 and rows[-1] == B - 1 and len(rows) >= 8
    want = encode_ref(sd, o[rows], cfg.n_poses, FID_VAE_LENGTH)
    err = _range_err(lat[rows], want)
    print(f"[measure] {ds} B={B}: encoder vs fp32 torch restatement on rows {rows}: max error / range = {err:.3e}")
    assert err <= 1e-3
    assert bool(torch.isfinite(lat).all())


@pytest.mark.parametrize("ds", ["show", "beat"])
def test_clip_in_batch_equals_clip_alone_and_later_frames_are_ignored(ds):
    cfg = get_config(ds)
    net, _ = fid_net(ds)
    outputs, _ = make_motion_pair(cfg, 70, 5)
    x = outputs.cuda()
    full = net(x)
    rng = float(full.max() - full.min())
    for b in (0, 33, 69):
        alone = net(x[b:b + 1])
        err = float((alone[0] - full[b]).abs().max()) / rng
        print(f"[measure] {ds}: clip {b} alone vs inside a batch of 70: {err:.2e} of range")
        assert err <= 1e-5          # (another M may pick another tile shape / kernel of the fp32 GEMM: round-off only)
    # frames beyond n_poses never reach the latent, whatever they hold — NaN included; the tensor ends right behind the last clip
    pad = torch.full((70, cfg.n_poses + 3, cfg.net_dim_pose), float("nan"), device="cuda")
    pad[:, :cfg.n_poses] = x
    assert torch.equal(net(pad), full)
    # exactly n_poses frames with NaN right behind the LAST clip in memory: the K pad of its last output row must not be read
    buf = torch.full((70 * cfg.n_poses * cfg.net_dim_pose + 4096,), float("nan"), device="cuda")
    buf[:x.numel()] = x.reshape(-1)
    assert torch.equal(net(buf[:x.numel()].view_as(x)), full)


def test_every_entry_point_is_bit_reproducible():
    cfg = get_config("show")
    net, _ = fid_net("show")
    outputs, motions = make_motion_pair(cfg, 120, 8)
    o, m = outputs.cuda(), motions.cuda()
    a, b = net(o), net(o)
    assert torch.equal(a, b)
    r1, r2 = metrics.batch_metrics(o, m, 1), metrics.batch_metrics(o, m, 1)
    for k in ("sq_sum", "pck_count", "mse", "pck", "diversity"):
        assert torch.equal(r1[k], r2[k]), k
    ob, mb = (t[..., :192].contiguous() for t in (o, m))
    r1, r2 = metrics.batch_metrics(ob, mb, 3), metrics.batch_metrics(ob, mb, 3)
    for k in ("sq_sum", "pck_count", "diversity"):
        assert torch.equal(r1[k], r2[k]), k


def test_channel_counts_that_are_no_multiple_of_four_and_64_frames():
    """Expression-only width (103) with the 64-frame network: the input is staged to a 4-aligned width, the rest is the same code."""
    import argparse
    opt = argparse.Namespace(n_poses=64, net_dim_pose=103, vae_length=32)
    sd = make_synthetic_fid_state_dict(opt, 7)
    net = metrics.HalfEmbeddingNet(opt, sd)
    x = torch.randn(9, 66, 103, generator=torch.Generator().manual_seed(1)).cuda()
    err = _range_err(net(x), encode_ref(sd, x, 64, 32))
    print(f"[measure] 103 channels, 64 frames, base 32: max error / range = {err:.3e}")
    assert err <= 1e-3


def test_refusals_launch_nothing():
    cfg = get_config("beat")
    L = _lib.lib()
    sd = make_synthetic_fid_state_dict(cfg, 1)
    h = metrics.create_fgd_handle(cfg.n_poses, cfg.net_dim_pose, FID_VAE_LENGTH)
    try:
        metrics.load_fgd_weights(h, {k: v for k, v in sd.items() if k != "pose_encoder.fc_mu.bias"})
        assert L.dsh_fgd_finalize(h) == -1 and b"pose_encoder.fc_mu.bias" in L.dsh_last_error()
        x = torch.zeros(2, cfg.n_poses, cfg.net_dim_pose, device="cuda")
        out = torch.zeros(2, FID_VAE_LENGTH, device="cuda")
        assert L.dsh_fgd_encode(h, x.data_ptr(), 2, cfg.n_poses, out.data_ptr()) == -1      # not finalized
    finally:
        L.dsh_fgd_destroy(h)
    net, _ = fid_net("beat")
    x = torch.ones(4, cfg.n_poses - 1, cfg.net_dim_pose, device="cuda")
    out = torch.full((4, FID_VAE_LENGTH), 7.0, device="cuda")
    torch.cuda.synchronize()
    _lib.launch_counts(reset=True)
    assert L.dsh_fgd_encode(net._h, x.data_ptr(), 4, cfg.n_poses - 1, out.data_ptr()) == -1
    assert b"n_poses = 34" in L.dsh_last_error()
    with pytest.raises(_lib.DshError, match="frames"):
        net(x)
    assert set(_lib.launch_counts().values()) == {0}
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    res = torch.zeros(4096, dtype=torch.float64, device="cuda")
    o = torch.zeros(4, 34, 192, device="cuda")
    for args in ((4, 34, 192, 2, 4), (4, 34, 192, 3, 1), (4, 34, 190, 3, 4), (4, 34, 192, 1, 5)):
        assert L.dsh_op_batch_metrics(None, o.data_ptr(), o.data_ptr(), *args, res.data_ptr()) == -1, args
    torch.cuda.synchronize()
    assert not bool(res.any())
    with pytest.raises(ValueError):
        metrics.batch_metrics(o[:1], o[:1], 3)


def test_validate_batch_equals_the_composition_by_hand():
    """validate_batch twice + validation_summary() on synthetic SHOW data = generate_batch, the encoder, batch_metrics, the meters and
    the Frechet distance composed by hand; the samples it returns are those of generate_batch alone with the same seed, bit for bit."""
    from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace
    cfg = get_config("show")
    model = gpu_model("show", "fp32")
    net, _ = fid_net("show")
    tr = DDPMTrainer(sampler_namespace(cfg), model, eval_model=net)
    plain = DDPMTrainer(sampler_namespace(cfg), model)
    assert tr.pck_joint_dim == 1 and DDPMTrainer(sampler_namespace(get_config("beat")), model).pck_joint_dim == 3
    L = cfg.overlap_len
    recs, outs = [], []
    for i, B in enumerate((3, 2)):
        inp = make_inputs(cfg, B, frames=cfg.n_poses, seed=40 + i)
        _, motions = make_motion_pair(cfg, B, 50 + i)
        cond = {"pretrain_aud_feat": inp["pretrain_aud_feat"]}
        got = tr.validate_batch(inp["audio_emb"], motions, inp["person_id"], cond, seed=77 + i)
        md = motions.cuda()
        mask = torch.zeros_like(md, dtype=torch.bool)
        mask[:, :L] = True
        want = plain.generate_batch(inp["audio_emb"], inp["person_id"], cfg.net_dim_pose, cond,
                                    {"gt": md, "outpainting_mask": mask, "outpainting_mask_any": True}, seed=77 + i)
        assert torch.equal(got, want), "adding the metrics to a validation step must leave its samples bit-identical"
        recs.append((metrics.batch_metrics(want, md, 1), net(want), net(md), B))
        outs.append(got)
    summary = tr.validation_summary()
    mse, pck, div = (metrics.AverageMeter(k) for k in ("mse", "pck", "div"))
    for r, _, _, B in recs:
        mse.update(float(r["mse"]), B)
        pck.update(float(r["pck"]), B)
        for d in r["diversity"].cpu().tolist():
            div.update(d, r["b_div"])
    fgd = metrics.frechet_distance(torch.cat([r[1] for r in recs]).cpu().numpy(), torch.cat([r[2] for r in recs]).cpu().numpy())
    print(f"[measure] validation summary {summary}")
    assert summary == {"MSE": mse.avg, "PCK": pck.avg, "Diversity": div.avg, "FGD": fgd}
    assert div.count == 5 and mse.count == 5
    # no eval_model: no FGD (--no_fgd); ragged batches are refused with a message
    inp = make_inputs(cfg, 2, frames=cfg.n_poses, seed=40)
    _, motions = make_motion_pair(cfg, 2, 50)
    plain.validate_batch(inp["audio_emb"], motions, inp["person_id"], {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, seed=1)
    assert set(plain.validation_summary()) == {"MSE", "PCK", "Diversity"}
    with pytest.raises(ValueError, match="full clips"):
        tr.validate_batch(inp["audio_emb"], motions, inp["person_id"], {}, lengths=[88, 40])
    with pytest.raises(ValueError, match="two clips"):
        tr.validate_batch(inp["audio_emb"][:1], motions[:1], inp["person_id"][:1], {})
