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
