"""Helpers of the ragged-batch tests (tests/test_ragged_cpu.py, tests/test_gpu_ragged.py): padded batches built from clips made alone
at their own length, the oracle with the three masks patched in, and a stub sampler that honours per-row lengths."""
from __future__ import annotations

import contextlib
from typing import Dict, List, Sequence

import torch
import torch.nn.functional as F

from diffsheg_amd.synthetic import make_inputs

GARBAGE = 1.0e4          # "large finite" content of padded frames


def clips_alone(cfg, lengths: Sequence[int], seed0: int = 10) -> List[Dict[str, torch.Tensor]]:
    """One independent clip per entry, made at its own length (batch 1 each)."""
    return [make_inputs(cfg, 1, frames=int(n), seed=seed0 + i) for i, n in enumerate(lengths)]


def pad_batch(clips: List[Dict[str, torch.Tensor]], key: str, frames: int, fill: float = 0.0) -> torch.Tensor:
    """[B, frames, ...] holding clip b's `key` in its first frames and `fill` behind them."""
    out = torch.full((len(clips), frames, clips[0][key].shape[-1]), float(fill))
    for i, c in enumerate(clips):
        out[i, :c[key].shape[1]] = c[key][0]
    return out


def person_ids(clips) -> torch.Tensor:
    return torch.cat([c["person_id"] for c in clips], 0)


@contextlib.contextmanager
def masked_oracle(lengths: Sequence[int], frames: int, attention: bool = True, conv1: bool = True, hubert_in: bool = True):
    """oracle.denoiser_ref with per-clip lengths patched in (in memory, for the duration of the block): frames >= length are excluded
    from the K softmax and k^T v of every linear attention (`attention`), read as zero by hubert_encoder's first convolution
    (`hubert_in`) and — conv1's output after BatchNorm + GELU — by its second one (`conv1`)."""
    from oracle import denoiser_ref as R
    B = len(lengths)
    mask = torch.zeros(B, frames)
    for i, n in enumerate(lengths):
        mask[i, :int(n)] = 1
    orig_attn, orig_hub = R.linear_self_attention, R.hubert_encoder

    def attn(sd, p, x, emb, n_head):
        if not attention:
            return orig_attn(sd, p, x, emb, n_head)
        Bx, Tx, D = x.shape
        m = mask.repeat(Bx // B, 1)[:, :, None].bool()
        n = R._ln(sd, p + ".norm", x)
        q = R._lin(sd, p + ".query", n).view(Bx, Tx, n_head, -1).softmax(dim=-1)
        k = torch.where(m, R._lin(sd, p + ".key", n), torch.full((), float("-inf"))).view(Bx, Tx, n_head, -1).softmax(dim=1)
        v = torch.where(m, R._lin(sd, p + ".value", n), torch.zeros(())).view(Bx, Tx, n_head, -1)
        att = torch.einsum("bnhd,bnhl->bhdl", k, v)
        y = torch.einsum("bnhd,bhdl->bnhl", q, att).reshape(Bx, Tx, D)
        return x + R.stylization(sd, p + ".proj_out", y, emb)

    def hub(sd, p, h):
        if hubert_in:
            h = torch.where(mask[:, :, None].bool(), h, torch.zeros(()))
        z = F.conv1d(h.transpose(1, 2), sd[p + ".0.weight"], None, padding=1)
        z = F.batch_norm(z, sd[p + ".1.running_mean"], sd[p + ".1.running_var"], sd[p + ".1.weight"], sd[p + ".1.bias"], False, 0.0, 1e-5)
        z = F.gelu(z)
        if conv1:
            z = torch.where(mask[:, None, :].bool(), z, torch.zeros(()))
        return F.conv1d(z, sd[p + ".3.weight"], None, padding=1).transpose(1, 2)

    R.linear_self_attention, R.hubert_encoder = attn, hub
    try:
        yield
    finally:
        R.linear_self_attention, R.hubert_encoder = orig_attn, orig_hub


def attention_ref(qkv: torch.Tensor, lengths: Sequence[int], head_dim: int) -> torch.Tensor:
    """The linear attention core on qkv [nb, T, 3D] (any float dtype, computed in fp64), clip b restricted to its first
    lengths[b % len(lengths)] frames for K and V; every one of the T query rows is answered."""
    nb, T, D3 = qkv.shape
    D, H = D3 // 3, D3 // 3 // head_dim
    x = qkv.double()
    q = x[..., :D].view(nb, T, H, head_dim).softmax(-1)
    out = torch.empty(nb, T, D, dtype=torch.float64)
    for b in range(nb):
        n = int(lengths[b % len(lengths)])
        k = x[b, :n, D:2 * D].view(n, H, head_dim).softmax(0)
        v = x[b, :n, 2 * D:].view(n, H, head_dim)
        att = torch.einsum("nhd,nhl->hdl", k, v)
        out[b] = torch.einsum("nhd,hdl->nhl", q[b], att).reshape(T, D)
    return out


def stub_trainer(cfg, calls=None):
    """DDPMTrainer with generate_batch replaced by a CPU function (the pattern of tests/test_seam_cpu.py): every output frame of a row
    depends on the row's key, the seed, its window of conditioning, its LENGTH and all of its pinned frames.  A row of a padded batch
    with `lengths` is computed from its first lengths[b] frames exactly as a batch of that row alone would be, and is 0 behind them —
    the definition of a ragged batch.  Everything above generate_batch is the product code."""
    from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace

    class Stub(DDPMTrainer):
        def __init__(self, opt):
            self.opt, self.device = opt, torch.device("cpu")

        def generate_batch(self, audio_emb, p_id, dim_pose, add_cond={}, inpaint_dict=None, seed=None, row_keys=None, lengths=None, **kw):
            B, T = audio_emb.shape[:2]
            if calls is not None:
                calls.append({"B": B, "T": T, "y": inpaint_dict, "seed": seed, "row_keys": list(row_keys),
                              "lengths": None if lengths is None else list(lengths), "kw": dict(kw)})
            out = torch.zeros(B, T, dim_pose)
            m_all = (inpaint_dict or {}).get("outpainting_mask")
            for b in range(B):
                n = T if lengths is None else int(lengths[b])
                g = torch.Generator().manual_seed((int(seed) * 1000003 + int(row_keys[b])) & ((1 << 62) - 1))
                o = (torch.randn(n, dim_pose, generator=g) + audio_emb[b, :n].mean(-1, keepdim=True)
                     + add_cond["pretrain_aud_feat"][b, :n].mean(-1, keepdim=True) + p_id[b].argmax() + 0.001 * n)
                if m_all is not None and bool(m_all.any()):
                    m, gt = m_all[b, :n], inpaint_dict["gt"][b, :n]
                    wt = torch.linspace(0.5, 1.5, n * dim_pose).view(n, dim_pose)
                    o = o + 0.01 * (gt * wt * m).sum()
                    o = torch.where(m, 0.5 * gt + 0.5 * o, o)
                    if kw.get("tail_blend"):
                        o = o + 0.125
                out[b, :n] = o
            return out
    return Stub(sampler_namespace(cfg))


def stream_inputs(cfg, N, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, N, cfg.audio_dim, generator=g), {"pretrain_aud_feat": torch.randn(1, N, 16, generator=g)},
            torch.eye(cfg.style_dim)[1:2])
