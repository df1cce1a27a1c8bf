"""Shared helpers for the parity tests."""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np
import torch

from diffsheg_amd.config import get_config
from diffsheg_amd.weights import make_synthetic_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WEIGHT_SEED = 1234


def golden(name: str):
    return np.load(os.path.join(GOLDEN, name))


@functools.lru_cache(maxsize=4)
def synthetic_sd(ds: str):
    return make_synthetic_state_dict(get_config(ds), WEIGHT_SEED)


_MODELS = {}


def gpu_model(ds: str, precision: str = "fp32", **cfg_over):
    """One UniDiffuser handle per (dataset, precision, overrides) for the whole test session."""
    from diffsheg_amd.model import UniDiffuser
    key = (ds, precision, tuple(sorted(cfg_over.items())))
    if key not in _MODELS:
        cfg = get_config(ds, **cfg_over)
        _MODELS[key] = UniDiffuser(cfg, synthetic_sd(ds), device="cuda:0", precision=precision)
    return _MODELS[key]


def gpu_single_model(precision: str = "fp32", ds: str = "show"):
    """The opt.unidiffuser = False model (runner.py:46-57): one MotionTransformer over all channels."""
    from diffsheg_amd.model import MotionTransformer
    key = (ds, precision, "single")
    if key not in _MODELS:
        cfg = get_config(ds, unidiffuser=False)
        _MODELS[key] = MotionTransformer(cfg, make_synthetic_state_dict(cfg, WEIGHT_SEED), device="cuda:0", precision=precision)
    return _MODELS[key]


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def max_abs(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def eval_call(model, cfg, inp, t, c1, c2):
    """one denoiser evaluation of make_inputs() data through the model handle; t / c1 / c2 scalars or per-clip tensors"""
    B, T = inp["x_T"].shape[:2]
    shape_e = (B, T, cfg.expression_dim)
    c1t = c1 if torch.is_tensor(c1) else torch.full((B,), float(c1))
    c2t = c2 if torch.is_tensor(c2) else torch.full((B,), float(c2))
    sa = [c1t.view(B, 1, 1).expand(shape_e), c2t.view(B, 1, 1).expand(shape_e)]
    tt = t if torch.is_tensor(t) else torch.full((B,), int(t), dtype=torch.long)
    return model(inp["x_T"].cuda(), tt.cuda(), sqrt_alphas=sa, audio_emb=inp["audio_emb"].cuda(),
                 length=torch.full((B,), T), person_id=inp["person_id"].cuda(),
                 add_cond={"pretrain_aud_feat": inp["pretrain_aud_feat"].cuda()}, pe_type="pe_sinu", y={})


class HOIST_CASE:
    """the batch of tests/test_gpu_eval.py's round-6 launch A/Bs (shared with tests/aud_hoist_worker.py)"""
    args = (720, 3.3, 3.1)

    @staticmethod
    def inputs(cfg):
        from diffsheg_amd.synthetic import make_inputs
        return make_inputs(cfg, 3, frames=88, seed=41)


def hoist_latched():
    """DSH_AUD_HOIST as this process's library has latched it (this read latches it if nothing has yet): 1 / 0"""
    from diffsheg_amd import _lib
    v = C.c_int64()
    _lib.check(_lib.lib().dsh_switch_read(b"DSH_AUD_HOIST", None, C.byref(v)))
    return int(v.value != 0)


# ---- precision "bf16x3" in the feature tests -----------------------------------------------------------------------------------------------
F32_STORAGE = ("fp32", "bf16x3")        # precisions with fp32 storage: the oracle gates of "fp32" (1e-3) hold for both


def assert_split_ran(counts, what=""):
    """a bf16x3 run above the few-row limit: its large Linears were on the split-bf16 loop, none on the exact-fp32 loop of gemm_f32_pro.hip"""
    assert counts["gemm_f32_split"] > 0 and counts["gemm_f32_pro"] == 0, (what, {k: counts[k] for k in ("gemm_f32_split", "gemm_f32_split_128", "gemm_f32_pro", "gemm_f32_fewrow")})


def philox_rows(seed, keys, n_row):
    """the first n_row normal draws of the row streams `keys` (dsh_op_philox_randn_rows): x_T of a loop sampled with row_keys, [len(keys), n_row] on the CPU"""
    from diffsheg_amd import _lib
    out = torch.empty(len(keys), n_row, device="cuda:0")
    karr = (C.c_uint64 * len(keys))(*[int(k) for k in keys])
    _lib.check(_lib.lib().dsh_op_philox_randn_rows(None, out.data_ptr(), len(keys), n_row, seed & (2 ** 64 - 1), 0, karr))
    return out.cpu()


def oracle_ddim25(sd, cfg, audio, hub, pid, xT, single=False):
    """The oracle's 25-step DDIM loop (oracle/sampler_ref.py, eta = 0) on CPU clips from a given x_T [n, T, C]: what a GPU loop that drew this
    x_T for these clips must reproduce within the loop gate of its precision."""
    from oracle import denoiser_ref, sampler_ref
    n = xT.shape[0]

    class _Src:                      # draw 0 = x_T; the randn_like of every ddim step is multiplied by sigma = 0
        i = 0

        def randn(self, shape):
            self.i += 1
            return xT.clone() if self.i == 1 else torch.zeros(*shape)

    def eps_fn(xc, t_orig, c1, c2):
        with torch.no_grad():
            tt = torch.full((n,), t_orig)
            if single:
                return denoiser_ref.single_motion_transformer(sd, cfg, xc, tt, audio, pid, hub)
            return denoiser_ref.unidiffuser(sd, cfg, xc, tt, c1, c2, audio, pid, hub)
    return sampler_ref.ddim_sample_loop(eps_fn, tuple(xT.shape), {}, _Src(), overlap_len=cfg.overlap_len)


def sub_batches(B, ns):
    """DenoiserContext: first_clip, clips [B i / ns, B (i + 1) / ns) of the ns sub-batch instances."""
    return [(B * i // ns, B * (i + 1) // ns) for i in range(ns)]


def sample_clips(B, T, ns, cap=10):
    """Clips of a batch of B clips of T frames on ns sub-batch streams to compare with the oracle: first and last clip, both sides of every
    sub-batch split, the first clips that straddle a 32-, 128- and 256-token block boundary, and two interior ones."""
    picks = [0, B - 1]
    for lo, _ in sub_batches(B, ns)[1:]:
        picks += [lo - 1, lo]
    for blk in (256, 128, 32):
        for b in range(1, B):
            if (b * T) // blk != ((b + 1) * T - 1) // blk and (b * T) % blk and b not in picks:
                picks.append(b)
                break
    picks += [B // 3, (5 * B) // 7]
    out = []
    for b in picks:
        if 0 <= b < B and b not in out:
            out.append(b)
    return out[:cap]
