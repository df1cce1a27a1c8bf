"""From-scratch restatements of the validation metrics for the tests (plain torch / numpy, keyed by the reference's state-dict names).
They share no code with the product path: the encoder is written with conv1d / batch_norm / linear on channel-first tensors with the
reference's channel-major flatten, i.e. none of the load-time transform (BatchNorm fold, tap repack, column permutation, K padding)
that csrc/pose_encoder.hip relies on."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from diffsheg_amd.weights import fid_out_net_layout


def encode_ref(sd, x: torch.Tensor, n_poses: int, base: int, dtype=torch.float32) -> torch.Tensor:
    """mu of HalfEmbeddingNet in eval mode for x [B, frames >= n_poses, C], on x's device, in `dtype`."""
    p = {k: v.to(device=x.device, dtype=dtype) for k, v in sd.items() if torch.is_floating_point(v) and k.startswith("pose_encoder.")}
    h = x[:, :n_poses].to(dtype).transpose(1, 2)
    for i, stride in enumerate((1, 1, 2)):
        k = f"pose_encoder.net.{i}"
        h = F.conv1d(h, p[k + ".0.weight"], p[k + ".0.bias"], stride=stride)
        h = F.batch_norm(h, p[k + ".1.running_mean"], p[k + ".1.running_var"], p[k + ".1.weight"], p[k + ".1.bias"], False, 0.0, 1e-5)
        h = F.leaky_relu(h, 0.2)
    h = F.conv1d(h, p["pose_encoder.net.3.weight"], p["pose_encoder.net.3.bias"])
    h = h.flatten(1)
    _, lin, bn = fid_out_net_layout(n_poses, base)
    for i, li in enumerate(lin):
        h = F.linear(h, p[f"pose_encoder.out_net.{li}.weight"], p[f"pose_encoder.out_net.{li}.bias"])
        if bn[i] >= 0:
            k = f"pose_encoder.out_net.{bn[i]}"
            h = F.batch_norm(h, p[k + ".running_mean"], p[k + ".running_var"], p[k + ".weight"], p[k + ".bias"], False, 0.0, 1e-5)
            if i > 0:
                h = F.leaky_relu(h, 1.0)       # nn.LeakyReLU(True): the positional argument is the negative slope, True == 1.0
    return F.linear(h, p["pose_encoder.fc_mu.weight"], p["pose_encoder.fc_mu.bias"])


def packed_forward(layers, x: torch.Tensor, n_poses: int, dim: int, dtype=torch.float64, mm=None) -> torch.Tensor:
    """The device computation on the host, in float64, from the packed layers of diffsheg_amd.metrics.packed_fgd_layers: channels-last
    activations, every conv as ONE matmul of the contiguous slices x[b, s t : s t + k, :] against [out, k * in], LeakyReLU(0.2) behind
    the first three, the last conv's output flattened as it lies, then plain Linears.
    dtype / mm: the same function in another precision and with another product, mm(a [rows, Kp], w [N, Kp]) -> a w^T (default: the plain
    matmul), e.g. float32 with one accumulator per output (f32_gates._mm) as the calibration of the derived gates."""
    mm = mm or (lambda a, w: a @ w.T)
    h = x[:, :n_poses].to(dtype)
    cp = layers[0][2] // 3                     # input channels as packed (padded to a multiple of 4)
    if cp != dim:
        h = F.pad(h, (0, cp - dim))
    for l, (ks, stride) in enumerate(((3, 1), (3, 1), (4, 2), (3, 1))):
        W, b, K = layers[l]
        assert K == ks * h.shape[2], (l, K, ks, h.shape)
        rows = h.unfold(1, ks, stride).permute(0, 1, 3, 2).reshape(h.shape[0], -1, K)       # [B, T_out, (tap, channel)]
        rows = F.pad(rows, (0, W.shape[1] - K))
        h = mm(rows.reshape(-1, W.shape[1]), torch.from_numpy(W).to(dtype)).reshape(rows.shape[0], rows.shape[1], -1) + torch.from_numpy(b).to(dtype)
        if l < 3:
            h = F.leaky_relu(h, 0.2)
    h = h.reshape(h.shape[0], -1)
    for W, b, K in layers[4:]:
        assert h.shape[1] == K
        h = mm(F.pad(h, (0, W.shape[1] - K)), torch.from_numpy(W).to(dtype)) + torch.from_numpy(b).to(dtype)
    return h


def batch_metrics_f64(outputs: torch.Tensor, motions: torch.Tensor, joint_dim: int, b_div: int) -> dict:
    """MSE, PCK count and per-group diversity in float64 on the tensors' device (torch.cdist(p=1) per group).  The difference itself is
    taken in float32, as the reference and the kernel take it (the inputs are float32 tensors), and everything behind it in float64.
    For joint_dim 1 the float32 test sqrt(d * d) < 0.5 is then EXACTLY |d| < 0.5 (d * d < 0.25 survives the rounding of the product
    on both sides of the threshold), so the counts must agree whatever the data; for joint_dim 3 the order of the float32 additions can
    decide a joint within ~1e-7 of the threshold: "pck_margin" reports the closest one."""
    o = outputs.double()
    B, T, C = o.shape
    d = (outputs.float() - motions.float()).double().reshape(B, T, C // joint_dim, joint_dim)
    root = (d ** 2).sum(-1).sqrt()
    divs = []
    for g in range(B // b_div):
        grp = o[g * b_div:(g + 1) * b_div].reshape(b_div, -1)
        dist = torch.cdist(grp, grp, p=1)
        divs.append(float(dist.triu(1).sum() / (T * C) * 2 / (b_div * (b_div - 1))))
    return {"mse": float((d ** 2).mean()), "pck_count": int((root < 0.5).sum()), "pck_total": root.numel(),
            "pck_margin": float((root - 0.5).abs().min()), "diversity": np.asarray(divs)}
