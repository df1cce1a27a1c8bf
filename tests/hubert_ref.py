"""CPU oracle of the HuBERT encoder (diffsheg_amd/csrc/hubert.hip): plain torch, dtype-generic, written from the architecture of transformers'
HubertModel in its hubert-large form (feat_extract_norm "layer", conv bias, stable LayerNorm) and pinned to it by
tests/golden/hubert_small.npz (test_hubert_cpu.py).  float64 is the reference; float32 is the calibration chain: every matrix product with one
accumulator per output, K ascending or descending (f32_gates._mm), torch's LayerNorm / GELU / softmax.

  1. x [B, n] normalised by the caller
  2. seven times Conv1d (valid, stride s, bias) -> LayerNorm over the channels of each frame (eps 1e-5) -> erf-GELU
  3. LayerNorm(conv_dim) -> Linear to hidden
  4. h += GELU(posconv(h)): Conv1d(hidden, hidden, pk, padding pk / 2, groups) with weight g v / |v| (norm over (out, in) per tap) and its LAST
     output frame dropped, so output t reads frames t - pk / 2 .. t + pk / 2 - 1, zeros outside
  5. per layer: h += out_proj(softmax(q k^T / 8) v) from LN(h); h += output_dense(GELU(intermediate_dense(final_LN(h))))
  6. encoder.layer_norm
"""
import numpy as np
import torch
import torch.nn.functional as F

import audio_ref
from f32_gates import _mm

LARGE = dict(hidden=1024, layers=24, heads=16, intermediate=4096, conv_dim=(512,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2),
             conv_stride=(5, 2, 2, 2, 2, 2, 2), pos_kernel=128, pos_groups=16, ln_eps=1e-5)
SMALL = dict(hidden=128, layers=2, heads=2, intermediate=256, conv_dim=(64,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2),
             conv_stride=(5, 2, 2, 2, 2, 2, 2), pos_kernel=16, pos_groups=2, ln_eps=1e-5)
POS = "encoder.pos_conv_embed.conv."
CHUNK = 320000


def num_frames(cfg, n):
    for k, s in zip(cfg["conv_kernel"], cfg["conv_stride"]):
        if n < k:
            return -1
        n = (n - k) // s + 1
    return n


def make_state_dict(cfg, seed, old_names=False):
    """A seeded state dict with HubertModel's keys and the initialisation scale of transformers (Linear / conv weights std 0.02, LayerNorm
    1 / 0) plus a spread on the biases and LayerNorm affines, so that no fold is trivially the identity."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, std=0.02: torch.randn(*s, generator=g) * std
    sd = {}
    cd, ck = cfg["conv_dim"], cfg["conv_kernel"]
    for i in range(7):
        k = f"feature_extractor.conv_layers.{i}."
        cin = cd[i - 1] if i else 1
        sd[k + "conv.weight"] = r(cd[i], cin, ck[i], std=(2.0 / (cin * ck[i])) ** 0.5)        # kaiming_normal_, as transformers initialises them
        sd[k + "conv.bias"] = r(cd[i], std=0.05)
        sd[k + "layer_norm.weight"] = 1 + r(cd[i], std=0.1)
        sd[k + "layer_norm.bias"] = r(cd[i], std=0.1)
    H, I = cfg["hidden"], cfg["intermediate"]
    sd["feature_projection.layer_norm.weight"] = 1 + r(cd[6], std=0.1)
    sd["feature_projection.layer_norm.bias"] = r(cd[6], std=0.1)
    sd["feature_projection.projection.weight"] = r(H, cd[6], std=(1.0 / cd[6]) ** 0.5)
    sd["feature_projection.projection.bias"] = r(H, std=0.05)
    cg, pk = H // cfg["pos_groups"], cfg["pos_kernel"]
    gk, vk = ("weight_g", "weight_v") if old_names else ("parametrizations.weight.original0", "parametrizations.weight.original1")
    v = r(H, cg, pk, std=2.0 * (1.0 / (pk * H)) ** 0.5)
    sd[POS + gk] = v.double().pow(2).sum((0, 1), keepdim=True).sqrt().float() * (1 + r(1, 1, pk, std=0.1))
    sd[POS + vk] = v
    sd[POS + "bias"] = r(H, std=0.05)
    for l in range(cfg["layers"]):
        k = f"encoder.layers.{l}."
        for pj in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[k + f"attention.{pj}.weight"] = r(H, H)
            sd[k + f"attention.{pj}.bias"] = r(H, std=0.05)
        for ln in ("layer_norm", "final_layer_norm"):
            sd[k + ln + ".weight"] = 1 + r(H, std=0.1)
            sd[k + ln + ".bias"] = r(H, std=0.1)
        sd[k + "feed_forward.intermediate_dense.weight"] = r(I, H)
        sd[k + "feed_forward.intermediate_dense.bias"] = r(I, std=0.05)
        sd[k + "feed_forward.output_dense.weight"] = r(H, I)
        sd[k + "feed_forward.output_dense.bias"] = r(H, std=0.05)
    sd["encoder.layer_norm.weight"] = 1 + r(H, std=0.1)
    sd["encoder.layer_norm.bias"] = r(H, std=0.1)
    return sd


def make_wave(n, seed):
    """a normalised test signal: unit normal samples with a slow envelope"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, generator=g) * (1 + 0.5 * torch.sin(torch.arange(n) * (2 * torch.pi / 997.0)))
    return (w - w.mean()) / torch.sqrt(w.var(unbiased=False) + 1e-7)


def pos_conv_weight(sd, dt=torch.float64):
    """[hidden, hidden / groups, k] = g v / |v|, norm over (out, in) per tap, in dtype dt"""
    g = sd.get(POS + "weight_g", sd.get(POS + "parametrizations.weight.original0")).to(dt)
    v = sd.get(POS + "weight_v", sd.get(POS + "parametrizations.weight.original1")).to(dt)
    return g * v / v.pow(2).sum((0, 1), keepdim=True).sqrt()


def conv_rows(x, k, s):
    """channels-last x [B, L, C] -> the im2col rows [B, (L - k) / s + 1, k C], tap-major"""
    B, L, C = x.shape
    return x.unfold(1, k, s).permute(0, 1, 3, 2).reshape(B, (L - k) // s + 1, k * C)


def conv_weight(w):
    """[out, in, k] -> [out, k in], tap-major"""
    return w.permute(0, 2, 1).reshape(w.shape[0], -1)


def conv_ln_gelu(x, w, b, gamma, beta, k, s, dt, reverse=False):
    rows = conv_rows(x.to(dt), k, s)
    y = _mm(rows.reshape(-1, rows.shape[-1]), conv_weight(w.to(dt)), reverse).reshape(rows.shape[0], rows.shape[1], -1) + b.to(dt)
    return F.gelu(F.layer_norm(y, (y.shape[-1],), gamma.to(dt), beta.to(dt), 1e-5))


def pos_conv(h, w, bias, groups, dt, reverse=False):
    """h [B, M, hidden] -> h + GELU(conv): w [hidden, cg, pk] the normalised weight"""
    B, M, H = h.shape
    cg, pk = w.shape[1], w.shape[2]
    hp = F.pad(h.to(dt), (0, 0, pk // 2, pk // 2 - 1))          # frames t - pk / 2 .. t + pk / 2 - 1: the last output frame is never formed
    rows = torch.stack([conv_rows(hp[:, :, g * cg:(g + 1) * cg], pk, 1).reshape(B * M, pk * cg) for g in range(groups)], 1)   # [B M, G, pk cg]
    wg = conv_weight(w.to(dt)).reshape(groups, cg, pk * cg)                                                                  # [G, out, pk cg]
    if dt != torch.float32:
        out = torch.einsum("mgk,gok->mgo", rows, wg)
    else:                                                       # one accumulator per output, K ascending (reverse: descending), all groups at once
        out = torch.zeros(B * M, groups, cg)
        wt = wg.permute(2, 0, 1).contiguous()
        for kk in (range(pk * cg - 1, -1, -1) if reverse else range(pk * cg)):
            out.addcmul_(rows[:, :, kk:kk + 1], wt[kk][None])
    return h.to(dt) + F.gelu(out.reshape(B, M, H) + bias.to(dt))


def features(sd, cfg, x, dt=torch.float64, reverse=False):
    """the convolution stack: x [B, n] -> [B, M, conv_dim[6]]"""
    h = x.to(dt)[:, :, None]
    for i in range(7):
        k = f"feature_extractor.conv_layers.{i}."
        h = conv_ln_gelu(h, sd[k + "conv.weight"], sd[k + "conv.bias"], sd[k + "layer_norm.weight"], sd[k + "layer_norm.bias"],
                         cfg["conv_kernel"][i], cfg["conv_stride"][i], dt, reverse)
    return h


def encode(sd, cfg, x, dt=torch.float64, reverse=False, fast=False):
    """last_hidden_state [B, M, hidden] of x [B, n] in dtype dt (on x's device).  fast: torch's own matmul and attention in place of the
    one-accumulator sums (scripts/audio_frontend_bench.py: what plain torch costs on the same device; not a calibration chain)."""
    T = lambda k: sd[k].to(device=x.device, dtype=dt)
    eps, H = cfg["ln_eps"], cfg["hidden"]
    mm = (lambda a, w, r: a @ w.T) if fast else _mm
    lin = lambda a, k: mm(a.reshape(-1, a.shape[-1]), T(k + ".weight"), reverse).reshape(a.shape[:-1] + (-1,)) + T(k + ".bias")
    ln = lambda a, k: F.layer_norm(a, (a.shape[-1],), T(k + ".weight"), T(k + ".bias"), eps)
    if fast:
        h = x.to(dt)[:, None, :]
        for i in range(7):
            k = f"feature_extractor.conv_layers.{i}."
            h = F.conv1d(h, T(k + "conv.weight"), T(k + "conv.bias"), stride=cfg["conv_stride"][i])
            h = F.gelu(F.layer_norm(h.transpose(1, 2), (h.shape[1],), T(k + "layer_norm.weight"), T(k + "layer_norm.bias"), 1e-5)).transpose(1, 2)
        h = lin(ln(h.transpose(1, 2), "feature_projection.layer_norm"), "feature_projection.projection")
        pk = cfg["pos_kernel"]
        w = pos_conv_weight({k: v.to(x.device) for k, v in sd.items() if k.startswith(POS)}, dt)
        h = h + F.gelu(F.conv1d(h.transpose(1, 2), w, T(POS + "bias"), padding=pk // 2, groups=cfg["pos_groups"])[:, :, :-1]).transpose(1, 2)
    else:
        h = features(sd, cfg, x, dt, reverse)
        h = lin(ln(h, "feature_projection.layer_norm"), "feature_projection.projection")
        h = pos_conv(h, pos_conv_weight(sd, dt), T(POS + "bias"), cfg["pos_groups"], dt, reverse)
    for l in range(cfg["layers"]):
        k = f"encoder.layers.{l}."
        a = ln(h, k + "layer_norm")
        q, kk, v = lin(a, k + "attention.q_proj"), lin(a, k + "attention.k_proj"), lin(a, k + "attention.v_proj")
        if fast:
            B, M = q.shape[:2]
            sp = lambda t: t.reshape(B, M, cfg["heads"], 64).transpose(1, 2)
            att = F.scaled_dot_product_attention(sp(q), sp(kk), sp(v)).transpose(1, 2).reshape(B, M, H)
        else:
            att = audio_ref.softmax_attention(torch.cat((q * 0.125, kk, v), -1), cfg["heads"], reverse)
        h = h + lin(att, k + "attention.out_proj")
        h = h + lin(F.gelu(lin(ln(h, k + "final_layer_norm"), k + "feed_forward.intermediate_dense")), k + "feed_forward.output_dense")
    return ln(h, "encoder.layer_norm")


def chunked(encode_fn, x):
    """get_hubert_from_16k_speech_long of the reference, restated: x [n] (normalised) -> [(n - 80) / 320, hidden].  Full chunks
    x[i c : i c + c + 80] for i < n / c (encoded as ONE batch), the remainder x[(n / c) c :] if it has at least 400 samples, concatenated, then cut
    or zero-padded to (n - 80) / 320 rows; the row counts may differ by one at most."""
    n, c = x.shape[0], CHUNK
    pieces = [x[i * c:i * c + c + 80] for i in range(n // c)]        # (a slice clamps: the last one is shorter when fewer than 80 samples follow)
    whole = [p for p in pieces if p.shape[0] == c + 80]
    parts = list(encode_fn(torch.stack(whole))) if whole else []
    parts += [encode_fn(p[None])[0] for p in pieces if p.shape[0] != c + 80]
    if n - (n // c) * c >= 400:
        parts.append(encode_fn(x[(n // c) * c:][None])[0])
    out = torch.cat(parts, 0)
    want = (n - 80) // 320
    if abs(out.shape[0] - want) > 1:
        raise ValueError(f"{out.shape[0]} encoder rows for {want} expected")
    if out.shape[0] < want:
        out = torch.cat((out, out.new_zeros(want - out.shape[0], out.shape[1])), 0)
    return out[:want]


def debug_kinds():
    return dict(CONV=0, FEAT_PROJ=1, POS_CONV=2, QKV=3, OUT_PROJ=4, FFN_IN=5, FFN_OUT=6)


def fold64(W, b, gamma, beta):
    """the pro 1 fold in float64: (W' = gamma (.) W, b' = b + W beta, fc = row sums of W' as rounded to fp32), all rounded to fp32"""
    Wf = (W.double() * gamma.double()).float()
    return Wf, (b.double() + W.double() @ beta.double()).float(), Wf.double().sum(1).float()
