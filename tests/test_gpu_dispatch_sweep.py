"""Evaluations and sampling loops on BOTH sides of every kernel-dispatch boundary, on a real MI355X.

The denoiser picks a kernel family per launch from the shape of the call (row counts, frames per window, clips per batch); the limits
live in denoiser.hip, denoiser_context.hip, loop_regime.h and the launchers.  This file mirrors those rules in plain Python (`expected_launches`; regime_rules.py), asks the
library which families actually ran (`dsh_debug_launch_counts`, host-side counters) and compares every case with the CPU oracle.  A
limit that moves in the C++ without moving here fails the counter assertion of the cases that straddle it, instead of silently
testing one side twice.

Tolerances are the project's own: FP32_ATOL / BF16_MAX / BF16_RMS of test_gpu_eval.py for one evaluation, and the loop gates of
test_gpu_sharded.py::test_full_batch_ddim25_loop_equals_its_rows_sampled_alone (1e-5 fp32 / 1.2e-2 bf16 against the rows sampled
alone, 1e-3 / 1.2e-2 against the oracle's loop).

Measured on an MI355X when this file was written (the tests print the figures): one evaluation against the oracle, worst clip over all
cases — bf16 max 2.5e-2 / rms 5.2e-3 in every regime (window-chain 2.49e-2, first generation 2.49e-2, fused FFN 2.40e-2, rolling
hi / lo 2.33e-2, row-major attention 2.36e-2; dense small grid 2.51e-2), fp32 max 7.2e-6; loops against the rows sampled alone — bf16
2.3e-3, fp32 6.4e-7, against the oracle's loop 4.4e-3 / 7.2e-7; guidance scale 1 at B = 140, unsplit vs two sub-batch streams 1.7e-3.
The whole file took about 70 s with its 91 bf16 / fp32 evaluation cases (18 s of it).

precision "bf16x3" is walked as a third precision with fp32's storage rules: `split_tile_128` restates the tile rule of the split-bf16
loop, `split_linears` / `expected_split_launches` every Linear an instance sends through the gemm() / gemm_pro() funnel, and both counters
(`gemm_f32_split`, `gemm_f32_split_128`) are compared exactly at every bf16x3 case — on either side of the 512-row limit, of the two stream
splits and of the three tile limits (N = 1 536 / 1 024 / 512).  Measured: worst |eps - oracle| 3.9e-5 with 64 x 64 tiles only (the
single-transformer model), 3.6e-5 with both tiles in one evaluation, 2.2e-6 at or below 512 rows (the fp32 kernels); with the 18 bf16x3
evaluation cases and the two bf16x3 dense grids the whole file takes 79 s, its 109 evaluation cases 22 s of it."""
import ctypes as C
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsheg_amd import _lib  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from oracle import denoiser_ref, sampler_ref  # noqa: E402
from regime_rules import GRAPH_ROWS, PIPE_ROWS, SPLIT, _loop_flags, n_streams  # noqa: E402,F401  (the stream split and the loop regime, restated there)
from test_gpu_eval import BF16_MAX, BF16_RMS, FP32_ATOL  # noqa: E402  (the evaluation gates, unchanged)
from util import WEIGHT_SEED, gpu_model, gpu_single_model, rel_err, sample_clips, sub_batches, synthetic_sd  # noqa: E402

LOOP_TOL = {"fp32": 1e-5, "bf16": 1.2e-2}            # a clip of a batched loop vs the clip sampled alone (test_gpu_sharded.py)
LOOP_ORACLE_TOL = {"fp32": 1e-3, "bf16": 1.2e-2}     # ... vs the oracle's 25-step loop from the same x_T

# ---------------------------------------------------------------------------------------------------------------------------------
# The dispatch rules, restated.  Every constant names where it lives; `expected_launches` is the only consumer.
# ---------------------------------------------------------------------------------------------------------------------------------
LAYERS = 8
TLS_ROWS = {"feat_proj.1": 2048, "qkv": 2560, "feat_proj.3": 3072, "ffn.linear2": 4096, "sty": 6144, "ffn.linear1": 6144}  # denoiser.hip kTlRoles: tls_rows
TLS_MAXCLIP, TL1_MAXCLIP, T2_MAXCLIP, FFN_MAXCLIP = 4, 6, 10, 3        # tl_small.hip, tl_common.h, tl2.hip, tl2.hip / tl3_ffn.hip
FFN_FUSE_ROWS = 128 * 64                                               # tl2.hip tl2_ffn_supported
HL_STY_ROWS, HL_F3_ROWS = 128 * 256, 128 * 128                         # denoiser.hip kTlRoles: hl_rows
ROLL_MIN_BLOCKS = 128                                                  # tl2.hip launch_tl2_linear: N split below this many token blocks
ATTN_MFMA_FRAMES = 96                                                  # denoiser.hip run_encoder
F32_PRECS = ("fp32", "bf16x3")
F32_FEWROW = 512                                                       # denoiser.hip f32_min_rows / gemm.hip ks_rows

SPLIT_TILE_BLOCKS = 256                                                # gemm_f32_split.hip launch_gemm_f32_split: 128 x 128 tiles where they fill 256 CUs

TL_FAMILIES = ("tl1", "tl2_loop", "tl2_roll", "tl2_roll_hl", "tl4", "tls", "ffn_fused", "ffn_fused_sty", "attn_mfma", "attn_rowmajor")


def _ceil_div(a, b):
    return (a + b - 1) // b


def _round_up(a, b):
    return _ceil_div(a, b) * b


def split_tile_128(M, N):
    """gemm_f32_split.hip launch_gemm_f32_split (`mi`): the 128 x 128 instantiation where its tiles fill the 256 CUs at least once, the
    64 x 64 one below.  The tile depends on N: q|k|v (N = 1 536, 12 column tiles) flips at M >= 2 689 rows, N = 1 024 at 3 969, N = 512 at 8 065."""
    return _ceil_div(M, 128) * _ceil_div(N, 128) >= SPLIT_TILE_BLOCKS


def doubled_rows(prec, doubled, Mc):
    """denoiser.hip run_encoder (r0): rows of a launch that carries both CFG halves.  The token-per-lane path starts the conditional half
    at the next 256-row block; fp32 storage ("fp32", "bf16x3") packs the halves: 2 Mc."""
    if not doubled:
        return Mc
    return _round_up(Mc, 256) + Mc if prec == "bf16" else 2 * Mc


def split_linears(kind, nb, T):
    """(name, N, rows) of every Linear ONE sub-batch instance of nb clips sends through the gemm() / gemm_pro() funnel for one conditioning
    and one evaluation with a timestep per clip (denoiser.hip; tests/split_gates.py MODEL_LINEARS names the line of each).  Under
    precision "bf16x3" the funnel launches the split loop for those with more than F32_FEWROW rows.  Not in the list, because the funnel's
    conditions send them to the tiled GEMM at any size: joint_embed, the motion encoders' time_embed.2, conv2 (no bias), encoder_aud's last
    Linear, pid_embed (one row per distinct speaker) and an `out` head whose width is no multiple of 4."""
    doubled = _doubled(kind)
    Mc = nb * T
    M = doubled_rows("bf16x3", doubled, Mc)
    cins = {"show": (103, 129), "beat": (51, 141), "single": (232,)}[kind]           # config.py: expression | gesture channels
    out = []
    for cin in cins:
        out += [("conv1", 128, Mc), ("time_embed.0", 2048, nb), ("film", LAYERS * 4 * 512, nb), ("audio_proj", 256, Mc)]
        for _ in range(LAYERS):
            out += [("feat_proj.1", 1024, Mc), ("feat_proj.3", 512, Mc), ("qkv", 1536, M), ("sty1.out", 512, M), ("ffn.linear1", 1024, M),
                    ("ffn.linear2", 512, M), ("sty2.out", 512, M)]
        if cin % 4 == 0:
            out.append(("out", cin, M))
    if kind != "single":                                                             # encoder_aud (D = 128) and UniDiffuser.time_embed
        out += [("aud.qkv", 384, Mc), ("aud_time_embed.0", 2048, nb), ("aud_time_embed.2", 2048, nb), ("aud_film", 512, nb),
                ("aud.sty1.out", 128, Mc), ("aud.ffn.linear1", 1024, Mc), ("aud.ffn.linear2", 128, Mc)]
    return out


def expected_split_launches(kind, B, T):
    """(split launches, those of them on the 128 x 128 tile) of ONE bf16x3 conditioning + evaluation, summed over its sub-batch instances:
    what `gemm_f32_split` and `gemm_f32_split_128` must read, both exactly."""
    total = big = 0
    for lo, hi in sub_batches(B, n_streams("bf16x3", B, T)):
        for _, N, rows in split_linears(kind, hi - lo, T):
            if rows > F32_FEWROW:
                total += 1
                big += int(split_tile_128(rows, N))
    return total, big


def refused(prec, B, T):
    """The shapes dsh_set_condition refuses (include/diffsheg_hip.h): the bf16 StylizationBlock launch fits neither the 32-token kernels
    (at most 4 clips per block) nor the first-generation ones (6 per 128-token block)."""
    return prec == "bf16" and min(31 // T + 2, B) > TLS_MAXCLIP and min(127 // T + 2, B) > TL1_MAXCLIP


def refused_before(prec, cfg_doubled, B, T):
    """The region the parent commit refused (from the middle of layer 0): the window-chain kernels only up to 6144 rows.  The predicate
    above may only shrink against this one."""
    if prec != "bf16" or min(127 // T + 2, B) <= TL1_MAXCLIP:
        return False
    Mc = B * T
    M = _round_up(Mc, 256) + Mc if cfg_doubled else Mc
    return not (min(31 // T + 2, B) <= TLS_MAXCLIP and M <= TLS_ROWS["sty"])


def _tl2_family(M, K):
    """launch_tl2_linear for the bf16-out instantiations with a rolling form (q|k|v, feat_proj.1, ffn.linear2): rolling loop when the
    token blocks alone fill the chip, else N split over grid.y on the round-2 loop."""
    return "tl2_roll" if _ceil_div(M, 256 if K == 512 else 128) >= ROLL_MIN_BLOCKS else "tl2_loop"


def expected_launches(kind, prec, doubled, B, T):
    """Token-per-lane / attention launches of ONE bf16 evaluation per family (exact), summed over its sub-batch streams."""
    out = {k: 0 for k in TL_FAMILIES}
    if prec != "bf16":
        return out
    n_enc = 1 if kind == "single" else 2
    for lo, hi in sub_batches(B, n_streams(prec, B, T)):
        nb = hi - lo
        Mc = nb * T
        M = _round_up(Mc, 256) + Mc if doubled else Mc
        tls_clips = min(31 // T + 2, nb) <= TLS_MAXCLIP
        tl1_clips = min(127 // T + 2, nb) <= TL1_MAXCLIP
        per_layer = []
        per_layer.append("tls" if Mc <= TLS_ROWS["feat_proj.1"] else _tl2_family(Mc, 1024))
        per_layer.append("tls" if Mc <= TLS_ROWS["feat_proj.3"] else ("tl2_roll_hl" if Mc >= HL_F3_ROWS else "tl1"))
        per_layer.append("tls" if M <= TLS_ROWS["qkv"] else _tl2_family(M, 512))
        per_layer.append("attn_mfma" if T <= ATTN_MFMA_FRAMES else "attn_rowmajor")
        if tls_clips and (M <= TLS_ROWS["sty"] or not tl1_clips):
            sty = "tls"
        elif M >= HL_STY_ROWS and min(255 // T + 2, nb) <= T2_MAXCLIP:
            sty = "tl2_roll_hl"
        else:
            sty = "tl1"
        per_layer.append(sty)
        if M >= FFN_FUSE_ROWS and min(127 // T + 2, nb) <= FFN_MAXCLIP:
            per_layer.append("ffn_fused")
        else:
            per_layer.append("tls" if M <= TLS_ROWS["ffn.linear1"] else "tl2_loop")          # (no rolling form of the GELU instantiation)
            per_layer.append("tls" if M <= TLS_ROWS["ffn.linear2"] else _tl2_family(M, 1024))
            per_layer.append(sty)
        for fam in per_layer:
            out[fam] += LAYERS * n_enc
        out["tl2_loop"] += n_enc                                                              # the `out` head (fp32 row-major output)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# The boundary table: one row per dispatch decision, with the cases that straddle it.  case = (model, precision, B, T);
# model: "show" / "beat" = UniDiffuser with that config (SHOW doubles the batch for CFG), "single" = MotionTransformer (SHOW config).
# `side(case)` says which side of the limit a case is on (derived from the shape, never from what ran); both sides must appear.
# ---------------------------------------------------------------------------------------------------------------------------------
def _doubled(model):
    return model in ("show", "single")


def _inst(case):
    """(Mc, M, nb) of the LARGEST sub-batch instance of the case."""
    model, prec, B, T = case
    lo, hi = max(sub_batches(B, n_streams(prec, B, T)), key=lambda r: r[1] - r[0])
    Mc = (hi - lo) * T
    return Mc, doubled_rows(prec, _doubled(model), Mc), hi - lo


def _smallest_show_batch_with_n512_on_the_large_tile(T=88):
    """The smallest SHOW batch whose largest instance, with the CFG doubling (2 Mc in fp32 storage), puts the N = 512 Linears on the
    128 x 128 tile — derived from the restated rules; it lies below the two-stream limit of 4096 conditional rows (46 x 88 = 4048)."""
    B = 1
    while not split_tile_128(_inst(("show", "bf16x3", B, T))[1], 512):
        B += 1
    return B


TILE512_B = _smallest_show_batch_with_n512_on_the_large_tile()
S, Bt, Sg = "show", "beat", "single"
BOUNDARIES = [
    dict(name="feat_proj.1: window-chain kernels up to 2048 rows", where="denoiser.hip kTlRoles tls_rows (TL_FEAT1)",
         side=lambda c: _inst(c)[0] <= 2048,
         cases=[(S, "bf16", 32, 64), (S, "bf16", 33, 64), (S, "bf16", 23, 88), (S, "bf16", 24, 88), (Bt, "bf16", 60, 34), (Bt, "bf16", 61, 34)]),
    dict(name="q|k|v: window-chain kernels up to 2560 rows", where="denoiser.hip kTlRoles tls_rows (TL_QKV)",
         side=lambda c: _inst(c)[1] <= 2560,
         cases=[(S, "bf16", 20, 64), (S, "bf16", 21, 64), (S, "bf16", 14, 88), (S, "bf16", 15, 88), (Bt, "bf16", 75, 34), (Bt, "bf16", 76, 34)]),
    dict(name="feat_proj.3 (hi/lo): window-chain kernels up to 3072 rows", where="denoiser.hip kTlRoles tls_rows (TL_FEAT3)",
         side=lambda c: _inst(c)[0] <= 3072,
         cases=[(S, "bf16", 48, 64), (S, "bf16", 49, 64), (S, "bf16", 34, 88), (S, "bf16", 35, 88), (Bt, "bf16", 90, 34), (Bt, "bf16", 91, 34)]),
    dict(name="ffn.linear2: window-chain kernels up to 4096 rows (also: reversed weight-stream order from 4096)", where="denoiser.hip kTlRoles tls_rows (TL_FFN2), tl() a.rev",
         side=lambda c: _inst(c)[1] <= 4096,
         cases=[(S, "bf16", 32, 64), (S, "bf16", 33, 64), (S, "bf16", 23, 88), (S, "bf16", 24, 88), (Bt, "bf16", 120, 34), (Bt, "bf16", 121, 34)]),
    dict(name="StylizationBlock / ffn.linear1: window-chain kernels up to 6144 rows", where="denoiser.hip kTlRoles tls_rows (TL_STY, TL_FFN1)",
         side=lambda c: _inst(c)[1] <= 6144,
         cases=[(S, "bf16", 48, 64), (S, "bf16", 49, 64), (S, "bf16", 34, 88), (S, "bf16", 35, 88), (Bt, "bf16", 180, 34), (Bt, "bf16", 181, 34),
                (Sg, "bf16", 34, 88), (Sg, "bf16", 35, 88)]),
    dict(name="window-chain FiLM prologue: at most 4 clips per 32-token block", where="tl_small.hip tls_film_clips_ok",
         side=lambda c: min(31 // c[3] + 2, c[2]) <= 4,
         cases=[(S, "bf16", b, t) for t in (10, 11, 15, 16) for b in (4, 5, 6)] + [(S, "bf16", 7, t) for t in (11, 15, 16)] +
               [(Bt, "bf16", b, t) for t in (5, 7, 10) for b in (1, 4, 6)]),
    dict(name="first-generation FiLM prologue: at most 6 clips per 128-token block (shorter windows stay on the window-chain kernels)",
         where="tl_linear.hip tl_linear_film_clips_ok, denoiser.hip tl_family()",
         side=lambda c: min(127 // c[3] + 2, c[2]) <= 6,
         cases=[(S, "bf16", 150, 25), (S, "bf16", 150, 26), (S, "bf16", 150, 24), (Bt, "bf16", 300, 25), (Bt, "bf16", 300, 26)]),
    dict(name="fused FFN launch from 8192 rows", where="tl2.hip tl2_ffn_supported",
         side=lambda c: _inst(c)[1] >= 8192,
         cases=[(S, "bf16", 63, 64), (S, "bf16", 64, 64), (S, "bf16", 46, 88), (S, "bf16", 47, 88), (Sg, "bf16", 46, 88), (Sg, "bf16", 47, 88)]),
    dict(name="fused FFN launch: at most 3 clips per 128-token block (T >= 64)", where="tl2.hip FFN_MAXCLIP, tl3_ffn.hip F3_MAXCLIP",
         side=lambda c: min(127 // c[3] + 2, _inst(c)[2]) <= 3,
         cases=[(S, "bf16", 70, 63), (S, "bf16", 70, 64)]),
    dict(name="rolling hi/lo kernels: StylizationBlock from 32768 rows, feat_proj.3 from 16384", where="denoiser.hip kTlRoles hl_rows, tl_family()",
         side=lambda c: _inst(c)[1] >= 32768,
         cases=[(S, "bf16", 510, 64), (S, "bf16", 512, 64), (S, "bf16", 372, 88), (S, "bf16", 374, 88)]),
    dict(name="rolling hi/lo StylizationBlock: at most 10 clips per 256-token block (T >= 29)", where="denoiser.hip tl_family() hl2_fits, tl2.hip T2_MAXCLIP",
         side=lambda c: min(255 // c[3] + 2, _inst(c)[2]) <= 10,
         cases=[(S, "bf16", 1180, 28), (S, "bf16", 1180, 29)]),
    dict(name="tl2 q|k|v (256-token blocks): N split over grid.y below 128 token blocks, rolling loop from there", where="tl2.hip launch_tl2_linear (mblocks)",
         side=lambda c: _ceil_div(_inst(c)[1], 256) >= 128,
         cases=[(S, "bf16", 504, 64), (S, "bf16", 506, 64)]),
    dict(name="tl2 feat_proj.1 (128-token blocks): N split over grid.y below 128 token blocks, rolling loop from there", where="tl2.hip launch_tl2_linear (mblocks)",
         side=lambda c: _ceil_div(_inst(c)[0], 128) >= 128,
         cases=[(S, "bf16", 508, 64), (S, "bf16", 510, 64)]),
    dict(name="MFMA attention up to 96 frames, row-major fallback above", where="denoiser.hip run_encoder (fr <= 96)",
         side=lambda c: c[3] <= 96,
         cases=[(S, "bf16", 5, 96), (S, "bf16", 5, 97), (S, "bf16", 5, 120)]),
    dict(name="bf16: two sub-batch streams from 12288 token rows", where="denoiser_context.hip min_rows_",
         side=lambda c: c[2] * c[3] >= 12288,
         cases=[(S, "bf16", 191, 64), (S, "bf16", 192, 64), (S, "bf16", 139, 88), (S, "bf16", 140, 88), (Sg, "bf16", 139, 88), (Sg, "bf16", 140, 88)]),
    dict(name="bf16: three sub-batch streams from 64500 token rows", where="denoiser_context.hip rows_per_stream_",
         side=lambda c: c[2] * c[3] >= 64500,
         cases=[(S, "bf16", 732, 88), (S, "bf16", 733, 88)]),
    dict(name="fp32: few-row K-split GEMM up to 512 rows, gemm_f32_pro above", where="denoiser.hip f32_min_rows, gemm.hip ks_rows",
         side=lambda c: c[2] * c[3] <= 512,
         cases=[(Bt, "fp32", 15, 34), (Bt, "fp32", 16, 34), (S, "fp32", 8, 64), (S, "fp32", 8, 65)]),
    dict(name="fp32: two sub-batch streams from 4096 token rows", where="denoiser_context.hip (precision 0)",
         side=lambda c: c[2] * c[3] >= 4096,
         cases=[(Bt, "fp32", 120, 34), (Bt, "fp32", 121, 34), (S, "fp32", 63, 65), (S, "fp32", 64, 64)]),
    dict(name="fp32: three sub-batch streams from 8700 token rows", where="denoiser_context.hip (precision 0)",
         side=lambda c: c[2] * c[3] >= 8700,
         cases=[(Bt, "fp32", 255, 34), (Bt, "fp32", 256, 34)]),
    # ---- precision "bf16x3": fp32 storage, the Linears of more than 512 rows on the split-bf16 loop (gemm_f32_split.hip)
    dict(name="bf16x3: the fp32 kernels up to 512 rows, the split loop above (a change of arithmetic)", where="denoiser.hip gemm() / f32_now(): f32_min_rows",
         side=lambda c: c[2] * c[3] <= 512,
         cases=[(Bt, "bf16x3", 15, 34), (Bt, "bf16x3", 16, 34), (S, "bf16x3", 8, 64), (S, "bf16x3", 8, 65)]),
    dict(name="bf16x3: two sub-batch streams from 4096 token rows", where="denoiser_context.hip (fp32 storage)",
         side=lambda c: c[2] * c[3] >= 4096,
         cases=[(Bt, "bf16x3", 120, 34), (Bt, "bf16x3", 121, 34), (S, "bf16x3", 63, 65), (S, "bf16x3", 64, 64)]),
    dict(name="bf16x3: three sub-batch streams from 8700 token rows", where="denoiser_context.hip (fp32 storage)",
         side=lambda c: c[2] * c[3] >= 8700,
         cases=[(Bt, "bf16x3", 255, 34), (Bt, "bf16x3", 256, 34)]),
    dict(name="bf16x3 q|k|v (N = 1536): 128 x 128 tile from 2689 rows", where="gemm_f32_split.hip launch_gemm_f32_split (mi)",
         side=lambda c: split_tile_128(_inst(c)[1], 1536),
         cases=[(Bt, "bf16x3", 79, 34), (Bt, "bf16x3", 80, 34), (Sg, "bf16x3", 15, 88), (Sg, "bf16x3", 16, 88)]),
    dict(name="bf16x3 feat_proj.1 / ffn.linear1 (N = 1024): 128 x 128 tile from 3969 rows", where="gemm_f32_split.hip launch_gemm_f32_split (mi)",
         side=lambda c: split_tile_128(_inst(c)[1], 1024),
         cases=[(Bt, "bf16x3", 116, 34), (Bt, "bf16x3", 117, 34)]),
    dict(name="bf16x3 N = 512 Linears (StylizationBlock with the CFG-null row constant, feat_proj.3, ffn.linear2): 128 x 128 tile from 8065 rows",
         where="gemm_f32_split.hip launch_gemm_f32_split (mi); denoiser.hip run_encoder: M = 2 Mc",
         side=lambda c: split_tile_128(_inst(c)[1], 512),
         cases=[(S, "bf16x3", TILE512_B - 1, 88), (S, "bf16x3", TILE512_B, 88)]),
]


def _ordered_cases():
    """Unique cases, grouped per context (model, precision), inside a group ordered so that shapes shrink and grow: the largest,
    the smallest, the second largest, ... — a context that keeps state from a larger or a smaller shape shows up in the next case."""
    uniq = sorted({c for row in BOUNDARIES for c in row["cases"]}, key=lambda c: (c[0], c[1], c[2] * c[3], c[3]))
    out = []
    for key in sorted({c[:2] for c in uniq}):
        grp = [c for c in uniq if c[:2] == key]
        while grp:
            out.append(grp.pop())
            if grp:
                out.append(grp.pop(0))
    return out


CASES = _ordered_cases()
PASSED = set()              # cases whose counter assertion, oracle comparison and whole-batch guard all passed
FIRST = {}                  # (model, precision) -> (case, eps of its first run)
WORST = {}                  # (precision, regime) -> worst measured error
T0 = [None]


def test_boundary_table_is_well_formed():
    """Pure bookkeeping (no GPU work): every row has cases on both sides of its limit, no sweep case is in the refused region, and the
    refused region did not grow against the parent's (dense grid included)."""
    T0[0] = time.time()
    for row in BOUNDARIES:
        sides = {bool(row["side"](c)) for c in row["cases"]}
        assert sides == {True, False}, (row["name"], sides)
    assert not [c for c in CASES if refused(c[1], c[2], c[3])]
    grid = [(m, p, b, t) for m in ("show", "beat") for p in ("bf16", "fp32", "bf16x3") for b in DENSE_B for t in DENSE_T] + CASES
    inside = [c for c in grid if refused(c[1], c[2], c[3])]
    before = [c for c in grid if refused_before(c[1], _doubled(c[0]), c[2], c[3])]
    assert set(inside) <= set(before)
    assert not [c for c in inside if c[1] in F32_PRECS]                       # fp32 storage refuses nothing, with either main loop
    # the bf16x3 rows: the tile limits are where the docstring of split_tile_128 puts them, the derived SHOW batch is the smallest one, every
    # bf16x3 case above the few-row limit has split launches to count, and the cases around the tile limits mix both instantiations
    assert [min(m for m in range(1, 20000) if split_tile_128(m, n)) for n in (1536, 1024, 512)] == [2689, 3969, 8065]
    assert TILE512_B * 88 < SPLIT["bf16x3"][0] and not split_tile_128(_inst(("show", "bf16x3", TILE512_B - 1, 88))[1], 512)
    x3 = [c for c in CASES if c[1] == "bf16x3"]
    assert {c[0] for c in x3} == {"show", "beat", "single"}
    for c in x3:
        total, big = expected_split_launches(c[0], c[2], c[3])
        assert (total > 0) == (_inst(c)[1] > F32_FEWROW) and 0 <= big <= total, (c, total, big)
    mixes = {c: expected_split_launches(c[0], c[2], c[3]) for c in x3}
    assert any(0 < big < total for total, big in mixes.values()) and any(big == 0 < total for total, big in mixes.values())
    print(f"[dispatch sweep] {len(CASES)} evaluation cases over {len(BOUNDARIES)} boundaries; refused region: {len(inside)} of {len(grid)} grid shapes "
          f"({100.0 * len(inside) / len(grid):.1f} %), was {len(before)} ({100.0 * len(before) / len(grid):.1f} %)")


# ---------------------------------------------------------------------------------------------------------------------------------
def _handle(model, prec):
    if model == "single":
        m = gpu_single_model(prec)
        from diffsheg_amd.weights import make_synthetic_state_dict
        return m, m.cfg, make_synthetic_state_dict(m.cfg, WEIGHT_SEED)
    return gpu_model(model, prec), get_config(model), synthetic_sd(model)


def _batch(cfg, B, T, seed):
    """B distinct clips of T frames with per-clip timesteps / coefficients (as test_gpu_eval.py::_big_batch)."""
    inp = make_inputs(cfg, B, frames=T, seed=seed)
    t = torch.tensor([(37 * i + 5) % 1000 for i in range(B)])
    c1 = 1.0 + 0.5 * (torch.arange(B, dtype=torch.float32) % 7) / 7
    c2 = 0.5 + 0.25 * (torch.arange(B, dtype=torch.float32) % 5) / 5
    return inp, t, c1, c2


def _eval(model, kind, cfg, inp, t, c1, c2):
    B, T = inp["x_T"].shape[:2]
    kw = dict(audio_emb=inp["audio_emb"].cuda(), length=torch.full((B,), T), person_id=inp["person_id"].cuda(),
              add_cond={"pretrain_aud_feat": inp["pretrain_aud_feat"].cuda()}, pe_type="pe_sinu", y={})
    if kind == "single":
        return model(inp["x_T"].cuda(), t.cuda(), **kw)
    shape_e = (B, T, cfg.expression_dim)
    return model(inp["x_T"].cuda(), t.cuda(), sqrt_alphas=[c1.view(B, 1, 1).expand(shape_e), c2.view(B, 1, 1).expand(shape_e)], **kw)


def _oracle(kind, sd, cfg, inp, t, c1, c2, rows):
    r = torch.tensor(rows)
    with torch.no_grad():
        if kind == "single":
            return denoiser_ref.single_motion_transformer(sd, cfg, inp["x_T"][r], t[r], inp["audio_emb"][r], inp["person_id"][r], inp["pretrain_aud_feat"][r])
        return denoiser_ref.unidiffuser(sd, cfg, inp["x_T"][r], t[r], c1[r].view(-1, 1, 1), c2[r].view(-1, 1, 1), inp["audio_emb"][r], inp["person_id"][r],
                                        inp["pretrain_aud_feat"][r])


def _sample_clips(prec, B, T, cap=10):
    """util.sample_clips on the sub-batch split the restated rules give this case."""
    return sample_clips(B, T, n_streams(prec, B, T), cap)


def _compare(prec, got, ref, rows, tag):
    """Per clip, the evaluation gates of test_gpu_eval.py.  Returns the worst (max, rms)."""
    wm = wr = 0.0
    for j, r in enumerate(rows):
        d = (got[j].double() - ref[j].double())
        e, rms = float(d.abs().max()), float(d.pow(2).mean().sqrt())
        wm, wr = max(wm, e), max(wr, rms)
        if prec in F32_PRECS:                             # bf16x3 claims the fp32 bar: the gate is the project's 1e-3, not a measurement
            assert e < FP32_ATOL, (tag, "clip", r, e)
        else:
            assert e < BF16_MAX and rms < BF16_RMS, (tag, "clip", r, e, rms)
    return wm, wr


def _regime(exp):
    return "+".join(k for k in ("tls", "tl1", "tl2_loop", "tl2_roll", "tl2_roll_hl", "ffn_fused", "attn_rowmajor") if exp.get(k))


def _run_case(case, seed=None):
    kind, prec, B, T = case
    model, cfg, sd = _handle(kind, prec)
    inp, t, c1, c2 = _batch(cfg, B, T, seed if seed is not None else 1000 + 7 * B + T)
    _lib.launch_counts(reset=True)
    eps = _eval(model, kind, cfg, inp, t, c1, c2)
    torch.cuda.synchronize()
    got = _lib.launch_counts()
    return model, cfg, sd, inp, t, c1, c2, eps.cpu(), got


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-B{c[2]}-T{c[3]}")
def test_evaluation_at_dispatch_boundary(case):
    """One evaluation of the case's shape: (1) the kernel families the restated rules predict are the ones that ran — exact launch
    counts on the bf16 path, the GEMM families and stream counts on fp32; (2) a sample of clips against the CPU oracle at the
    evaluation gates; (3) the whole-batch guard of test_eval_bf16_headline_batch_sampled_clips_match_oracle on the other clips."""
    kind, prec, B, T = case
    model, cfg, sd, inp, t, c1, c2, eps, got = _run_case(case)
    # (1)
    assert got["eval_streams"] == n_streams(prec, B, T), (case, got)
    exp = expected_launches(kind, prec, _doubled(kind), B, T)
    assert {k: got[k] for k in TL_FAMILIES} == exp, (case, {k: (got[k], exp[k]) for k in TL_FAMILIES if got[k] != exp[k]})
    if prec != "bf16x3":
        assert got["gemm_f32_split"] == 0 and got["gemm_f32_split_128"] == 0, (case, got)
    else:
        # the split launches and their tile, both exactly as the restated rules give them; no exact-fp32 gemm_f32_pro launch at any size
        # (at or below the few-row limit the fp32 kernels run: the few-row K-split GEMM, as for "fp32")
        want = expected_split_launches(kind, B, T)
        print(f"[dispatch sweep {case}] split launches (all, 128 x 128): counted {(got['gemm_f32_split'], got['gemm_f32_split_128'])}, restated rules {want}")
        assert (got["gemm_f32_split"], got["gemm_f32_split_128"]) == want, (case, got, want)
        assert got["gemm_f32_pro"] == 0, (case, got)
        if B * T <= F32_FEWROW and not _doubled(kind):
            assert got["gemm_f32_split"] == 0 and got["gemm_f32_fewrow"] > 0 and got["gemm_f32_tiled"] == 0, (case, got)
        SPLIT_SEEN[case] = (got["gemm_f32_split"], got["gemm_f32_fewrow"])
    if prec in F32_PRECS:
        EPS_SEEN[case] = eps
    if prec == "fp32":
        # (Linears of at most 16 rows — the embeddings of a small batch — take the weight-streaming kernel, which is none of the three)
        if B * T <= F32_FEWROW and not _doubled(kind):
            assert got["gemm_f32_fewrow"] > 0 and got["gemm_f32_pro"] == 0 and got["gemm_f32_tiled"] == 0, (case, got)
        if B * T > F32_FEWROW:
            assert got["gemm_f32_pro"] > 0, (case, got)
        FEWROW_SEEN[case] = got["gemm_f32_fewrow"]
    # (2)
    rows = _sample_clips(prec, B, T)
    ref = _oracle(kind, sd, cfg, inp, t, c1, c2, rows)
    wm, wr = _compare(prec, eps[torch.tensor(rows)], ref, rows, case)
    # (3)
    assert torch.isfinite(eps).all()
    if B >= 3:
        per_clip = eps.abs().mean(dim=(1, 2))
        med = float(per_clip.median())
        assert float(per_clip.max()) < 3.0 * med and float(per_clip.min()) > 0.3 * med, (case, float(per_clip.min()), med, float(per_clip.max()))
    if prec == "bf16x3":
        mix = "none" if not want[0] else "64 x 64" if not want[1] else "128 x 128" if want[1] == want[0] else "mixed"
        reg = (prec, f"streams={got['eval_streams']},tiles={mix}")
    else:
        reg = (prec, _regime(exp) if prec == "bf16" else f"streams={got['eval_streams']},pro={int(got['gemm_f32_pro'] > 0)}")
    WORST[reg] = max(WORST.get(reg, (0.0, 0.0)), (wm, wr))
    print(f"[dispatch sweep {case}] families {reg[1]}; {len(rows)} clips {rows}: max|eps-ref| = {wm:.3e}, rms = {wr:.3e}")
    FIRST.setdefault((kind, prec), (case, eps))
    PASSED.add(case)


FEWROW_SEEN = {}
SPLIT_SEEN = {}             # bf16x3 case -> (split launches, few-row launches)
EPS_SEEN = {}               # fp32-storage case -> eps of its sweep run


def test_fp32_few_row_gemm_boundary_with_cfg():
    """SHOW fp32 doubles the batch, so launches of both CFG halves are above 512 rows on either side; what crosses the limit is the
    conditional-half launches (feat_proj.1 / feat_proj.3: 2 per layer and encoder, and the embedding of x): at 8 x 64 = 512 rows they take
    the few-row K-split GEMM, at 8 x 65 = 520 they do not."""
    a, b = ("show", "fp32", 8, 64), ("show", "fp32", 8, 65)
    assert a in FEWROW_SEEN and b in FEWROW_SEEN, "the sweep cases did not run"
    assert FEWROW_SEEN[a] - FEWROW_SEEN[b] >= 2 * LAYERS * 2, (FEWROW_SEEN[a], FEWROW_SEEN[b])


def test_bf16x3_few_row_boundary():
    """BEAT (no doubling): at 15 x 34 = 510 rows no launch is on the split loop and eps is the fp32 context's eps for the same case bit for
    bit; at 16 x 34 = 544 every funnel Linear is split and eps is no longer the fp32 bits (the arithmetic changed: were it equal, the
    split loop would not have run).
    SHOW doubles the batch: at 8 x 64 = 512 conditional rows the launches that carry both CFG halves (1 024 rows: q|k|v, the two
    StylizationBlock Linears and the FFN, 5 per layer and encoder) are on the split loop already - exactly those, by the exact count of the
    sweep case - and the conditional-half launches (feat_proj.1 / feat_proj.3, audio_proj, encoder_aud) still take the few-row kernels; at
    8 x 65 = 520 rows they cross as well.  So neither SHOW case equals fp32 bit for bit."""
    lo, hi = ("beat", "bf16x3", 15, 34), ("beat", "bf16x3", 16, 34)
    a, b = ("show", "bf16x3", 8, 64), ("show", "bf16x3", 8, 65)
    for c in (lo, hi, a, b):
        assert c in SPLIT_SEEN and (c[0], "fp32", c[2], c[3]) in EPS_SEEN, "the sweep cases did not run"
    f32 = lambda c: EPS_SEEN[(c[0], "fp32", c[2], c[3])]
    assert SPLIT_SEEN[lo][0] == 0 and torch.equal(EPS_SEEN[lo], f32(lo))
    assert SPLIT_SEEN[hi][0] > 0 and not torch.equal(EPS_SEEN[hi], f32(hi))
    assert SPLIT_SEEN[a][0] == 2 * LAYERS * 5, SPLIT_SEEN[a]
    assert SPLIT_SEEN[b][0] - SPLIT_SEEN[a][0] >= 2 * LAYERS * 2 and SPLIT_SEEN[a][1] - SPLIT_SEEN[b][1] >= 2 * LAYERS * 2, (SPLIT_SEEN[a], SPLIT_SEEN[b])
    assert not torch.equal(EPS_SEEN[a], f32(a)) and not torch.equal(EPS_SEEN[b], f32(b))
    for c in (hi, a, b):
        d = float((EPS_SEEN[c].double() - f32(c).double()).abs().max())
        print(f"[dispatch sweep {c}] max |eps(bf16x3) - eps(fp32)| = {d:.3e}")


@pytest.mark.parametrize("key", sorted({c[:2] for c in CASES}), ids=lambda k: f"{k[0]}-{k[1]}")
def test_context_carries_no_state_through_the_regimes(key):
    """After a context has walked through every regime of the sweep, its first case evaluates bit-identically to its first run.  (A bf16x3
    context has alternated between the fp32 weights and their packed copies on the way: its cases are ordered large, small, large, ...)"""
    assert key in FIRST, "the sweep cases of this context did not run"
    case, eps0 = FIRST[key]
    *_, eps, got = _run_case(case)
    assert torch.equal(eps, eps0), (case, float((eps - eps0).abs().max()))


def test_every_boundary_has_a_passing_case_on_each_side():
    for row in BOUNDARIES:
        ok = {bool(row["side"](c)) for c in row["cases"] if c in PASSED}
        assert ok == {True, False}, (row["name"], row["where"], [c for c in row["cases"] if c not in PASSED])
    for (prec, reg), (wm, wr) in sorted(WORST.items()):
        print(f"[dispatch sweep worst] {prec} {reg}: max {wm:.3e} rms {wr:.3e}")
    if T0[0]:
        print(f"[dispatch sweep] evaluation sweep wall time {time.time() - T0[0]:.1f} s")


# ---------------------------------------------------------------------------------------------------------------------------------
# The refused region
# ---------------------------------------------------------------------------------------------------------------------------------
DENSE_B = (1, 4, 5, 6, 7, 8, 40, 150)
DENSE_T = (1, 5, 7, 10, 11, 15, 16, 20, 25, 26)


@pytest.mark.parametrize("ds,prec", [("show", "bf16"), ("beat", "bf16"), ("show", "fp32"), ("beat", "fp32"), ("show", "bf16x3"), ("beat", "bf16x3")])
def test_dense_small_grid_is_evaluated_or_refused_cleanly(ds, prec):
    """Every (B, T) of the dense grid on ONE context per dataset and precision, in an order that alternates large and small: a shape
    outside the predicate is never refused and matches the oracle (all clips up to 8, a sample above) with the launches the rules
    predict; a shape inside it raises from the Python shim with a message that names the limit — and the evaluations that follow on
    the same context keep matching the oracle.  fp32 storage refuses nothing, with either main loop ("fp32", "bf16x3"); for bf16x3 the grid
    crosses the 512-row limit back and forth on one context, and the split launches are counted against the restated rules at every shape."""
    model, cfg, sd = _handle(ds, prec)
    shapes = sorted(((b, t) for b in DENSE_B for t in DENSE_T), key=lambda s: (s[0] * s[1], s[0]))
    order = []
    while shapes:
        order.append(shapes.pop())
        if shapes:
            order.append(shapes.pop(0))
    n_ref, worst, fails = 0, (0.0, 0.0), []
    for B, T in order:
        inp, t, c1, c2 = _batch(cfg, B, T, 5000 + 31 * B + T)
        if refused(prec, B, T):
            n_ref += 1
            with pytest.raises((RuntimeError, ValueError), match="at most 6 clips"):
                _eval(model, ds, cfg, inp, t, c1, c2)
            continue
        try:
            _lib.launch_counts(reset=True)
            eps = _eval(model, ds, cfg, inp, t, c1, c2).cpu()
            got = _lib.launch_counts()
            exp = expected_launches(ds, prec, _doubled(ds), B, T)
            assert {k: got[k] for k in TL_FAMILIES} == exp, {k: (got[k], exp[k]) for k in TL_FAMILIES if got[k] != exp[k]}
            if prec == "bf16x3":
                assert (got["gemm_f32_split"], got["gemm_f32_split_128"]) == expected_split_launches(ds, B, T) and got["gemm_f32_pro"] == 0, got
            assert torch.isfinite(eps).all()
            rows = list(range(B)) if B <= 8 else _sample_clips(prec, B, T, cap=8)
            ref = _oracle(ds, sd, cfg, inp, t, c1, c2, rows)
            worst = max(worst, _compare(prec, eps[torch.tensor(rows)], ref, rows, (ds, prec, B, T)))
        except (AssertionError, RuntimeError) as e:
            fails.append(((B, T), repr(e)[:300]))
    print(f"[dense grid {ds} {prec}] {len(order)} shapes, {n_ref} refused ({100.0 * n_ref / len(order):.1f} %), worst max|eps-ref| = {worst[0]:.3e} rms = {worst[1]:.3e}")
    assert not fails, fails
    assert n_ref == (sum(1 for b in DENSE_B for t in DENSE_T if b >= 7 and t <= 10) if prec == "bf16" else 0)


def _loop_inputs(cfg, B, T, seed=19):
    small = make_inputs(cfg, min(B, 64), frames=T, seed=seed)
    rep = (B + 63) // 64
    audio = small["audio_emb"].repeat(rep, 1, 1)[:B].cuda().contiguous()
    hub = small["pretrain_aud_feat"].repeat(rep, 1, 1)[:B].cuda().contiguous()
    audio += 0.01 * torch.randn(audio.shape, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(2))
    pid = torch.zeros(B, cfg.style_dim, device="cuda:0")
    pid[torch.arange(B), torch.arange(B) % cfg.style_dim] = 1.0
    return audio, hub, pid


def _refused_sample(tr, model, B, T):
    """dsh_sample on the current condition with DSH_NOISE_STACK and no stack: refused by an argument check that sits behind loop_begin."""
    opts = tr.diffusion_ddim_val._opts(0, False, 0, 5)
    x = torch.zeros(B, T, model.cfg.net_dim_pose, device="cuda:0")
    rc = _lib.lib().dsh_sample(model._h, C.byref(opts), x.data_ptr(), 0, None, None, 0, None, 0, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("ds", ["show", "beat"])
def test_context_is_intact_after_a_refusal(ds):
    """A refused evaluation and a refused sampling loop leave the context as it was: the same context then evaluates a supported shape,
    and samples a supported loop, bit-identically to a context that never saw the refused shape; the caller's stream stays ordered
    (the shim leaves the context stream in a `finally`)."""
    from diffsheg_amd.model import UniDiffuser
    cfg, sd = get_config(ds), synthetic_sd(ds)
    Cc = cfg.net_dim_pose
    good = _batch(cfg, 6, 7, 71)
    bad = _batch(cfg, 8, 7, 72)
    la, lh, lp = _loop_inputs(cfg, 5, 20)
    ba, bh, bp = _loop_inputs(cfg, 8, 9)

    def loop(tr):
        return tr.generate_batch(la, lp, Cc, {"pretrain_aud_feat": lh}, {}, seed=5, row_keys=list(range(5))).clone()

    fresh = UniDiffuser(cfg, sd, device="cuda:0", precision="bf16")
    want_eval = _eval(fresh, ds, cfg, *good).clone()
    want_loop = loop(DDPMTrainer(sampler_namespace(cfg), fresh))
    del fresh
    model = UniDiffuser(cfg, sd, device="cuda:0", precision="bf16")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                  # (a caller on another stream: _enter / _exit order the two)
        with pytest.raises(RuntimeError, match="at most 6 clips"):
            _eval(model, ds, cfg, *bad)
    side.synchronize()
    assert torch.equal(_eval(model, ds, cfg, *good), want_eval)
    with pytest.raises(RuntimeError, match="at most 6 clips"):
        tr.generate_batch(ba, bp, Cc, {"pretrain_aud_feat": bh}, {}, seed=5, row_keys=list(range(8)))
    assert torch.equal(loop(tr), want_loop)
    # a call that dsh_sample itself refuses after it has begun the loop (a noise-stack run without a stack) ends the loop state too
    assert _refused_sample(tr, model, 5, 20) < 0
    assert torch.equal(loop(tr), want_loop)
    assert torch.equal(_eval(model, ds, cfg, *good), want_eval)
    del tr, model


# ---------------------------------------------------------------------------------------------------------------------------------
# Loops at the loop thresholds
# ---------------------------------------------------------------------------------------------------------------------------------
def _philox_rows(seed, keys, n_row):
    out = torch.empty(len(keys), n_row, device="cuda:0")
    karr = (C.c_uint64 * len(keys))(*[int(k) for k in keys])
    _lib.check(_lib.lib().dsh_op_philox_randn_rows(None, out.data_ptr(), len(keys), n_row, seed & (2 ** 64 - 1), 0, karr))
    return out.cpu()


def _picks(B):
    """Around every possible stream split, and the batch ends (test_gpu_sharded.py)."""
    return sorted({b for b in (0, 1, B // 3 - 1, B // 3, B // 3 + 1, B // 2 - 1, B // 2, 2 * B // 3 - 1, 2 * B // 3 + 1, B - 2, B - 1) if 0 <= b < B})


LOOP_CASES = [
    # (model, precision, B, DSH_PIPE, sampler)
    ("show", "bf16", 46, "1", "ddim"), ("show", "bf16", 47, "1", "ddim"),            # graphs on | off
    ("show", "bf16", 732, "1", "ddim"), ("show", "bf16", 733, "1", "ddim"),          # pipeline on one batch | three sub-batch streams
    ("show", "bf16", 139, "0", "ddim"), ("show", "bf16", 140, "0", "ddim"),          # one | two sub-batch streams
    ("single", "bf16", 139, "1", "ddim"), ("single", "bf16", 140, "1", "ddim"),      # the same on the single MotionTransformer
    ("beat", "fp32", 120, "0", "ddim"), ("beat", "fp32", 121, "0", "ddim"), ("beat", "fp32", 121, "1", "ddim"),
    ("beat", "fp32", 255, "0", "ddim"), ("beat", "fp32", 255, "1", "ddim"),
    ("show", "bf16", 140, "0", "ddpm50"),
]


@pytest.mark.parametrize("kind,prec,B,pipe_env,sampler", LOOP_CASES, ids=lambda v: str(v))
def test_loop_at_threshold_equals_its_rows_sampled_alone(kind, prec, B, pipe_env, sampler, monkeypatch):
    """A whole sampling loop on either side of a loop threshold, one Philox stream per clip: the graph / pipeline / stream flags are
    the ones the rules predict, clips around every split and at the batch ends equal the clip sampled alone, and (ddim25) two clips
    equal the oracle's 25-step loop started from the x_T the GPU drew for them."""
    monkeypatch.setenv("DSH_PIPE", pipe_env)
    model, cfg, sd = _handle(kind, prec)
    ddim = sampler == "ddim"
    tr = DDPMTrainer(sampler_namespace(cfg, ddim=ddim, diffusion_steps=cfg.diffusion_steps if ddim else 50), model)
    T, Cc = cfg.n_poses, cfg.net_dim_pose
    audio, hub, pid = _loop_inputs(cfg, B, T)
    keys = list(range(1000, 1000 + B))
    _lib.launch_counts(reset=True)
    full = tr.generate_batch(audio, pid, Cc, {"pretrain_aud_feat": hub}, {}, seed=77, row_keys=keys)
    torch.cuda.synchronize()
    got = _lib.launch_counts()
    assert full.shape == (B, T, Cc) and torch.isfinite(full).all()
    graph, pipe, streams = _loop_flags(B, T, prec, kind, pipe_env == "1", ddim)
    assert (got["sample_graph"], got["sample_pipe"], got["sample_streams"]) == (graph, pipe, streams), (got, (graph, pipe, streams))
    full = full.clone()
    worst = 0.0
    for b in _picks(B):
        solo = tr.generate_batch(audio[b:b + 1], pid[b:b + 1], Cc, {"pretrain_aud_feat": hub[b:b + 1]}, {}, seed=77, row_keys=[keys[b]])
        worst = max(worst, rel_err(solo[0], full[b]))
    print(f"[loop {kind} {prec} B={B} DSH_PIPE={pipe_env} {sampler}] graph/pipe/streams = {graph}/{pipe}/{streams}; worst rel err vs the clip sampled alone: {worst:.3e}")
    assert worst < LOOP_TOL[prec]
    if not ddim:
        return
    ocl = [0, B - 1]
    a_c, h_c, p_c = audio[ocl].cpu(), hub[ocl].cpu(), pid[ocl].cpu()
    xT = _philox_rows(77, [keys[b] for b in ocl], T * Cc).view(len(ocl), T, Cc)

    class _Src:                      # draw 0 = x_T; the randn_like of every ddim step is multiplied by sigma = 0
        i = 0

        def randn(self, shape):
            self.i += 1
            return xT.clone() if self.i == 1 else torch.zeros(*shape)

    def eps_fn(xc, t_orig, c1, c2):
        with torch.no_grad():
            tt = torch.full((len(ocl),), t_orig)
            if kind == "single":
                return denoiser_ref.single_motion_transformer(sd, cfg, xc, tt, a_c, p_c, h_c)
            return denoiser_ref.unidiffuser(sd, cfg, xc, tt, c1, c2, a_c, p_c, h_c)
    xr = sampler_ref.ddim_sample_loop(eps_fn, (len(ocl), T, Cc), {}, _Src(), overlap_len=cfg.overlap_len)
    eo = max(rel_err(full[b], xr[j]) for j, b in enumerate(ocl))
    print(f"[loop {kind} {prec} B={B}] clips {ocl} vs the oracle's 25-step loop from the same x_T: max err / range {eo:.3e}")
    assert eo < LOOP_ORACLE_TOL[prec]


def test_mid_size_loop_is_bit_identical_pipelined_split_and_traced(monkeypatch):
    """SHOW bf16, B = 200 (17 600 clip rows): the two-encoder pipeline on one batch (default), two sub-batch streams (DSH_PIPE=0) and the
    unsplit loop without the pipeline (return_trace) give the same sample bit for bit — with CFG doubling the batch and its halves are
    all above the fused-FFN limit, so every clip runs the same kernels in all three."""
    model, cfg, sd = _handle("show", "bf16")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B, T, Cc = 200, cfg.n_poses, cfg.net_dim_pose
    audio, hub, pid = _loop_inputs(cfg, B, T, seed=23)
    keys = list(range(300, 300 + B))
    outs = {}
    for tag, env, kw in (("pipe", "1", {}), ("split", "0", {}), ("trace", "1", {"return_trace": True})):
        monkeypatch.setenv("DSH_PIPE", env)
        _lib.launch_counts(reset=True)
        # (new tensor objects: the shim conditions the context again, which is where the split is decided under the current switch)
        r = tr.generate_batch(audio.clone(), pid.clone(), Cc, {"pretrain_aud_feat": hub.clone()}, {}, seed=11, row_keys=keys, **kw)
        torch.cuda.synchronize()
        got = _lib.launch_counts()
        outs[tag] = (r[0] if kw else r).clone()
        want = _loop_flags(B, T, "bf16", "show", env == "1", trace=bool(kw))
        assert (got["sample_graph"], got["sample_pipe"], got["sample_streams"]) == want, (tag, got, want)
        assert got["ffn_fused"] > 0, (tag, got)
    assert torch.isfinite(outs["pipe"]).all()
    assert torch.equal(outs["pipe"], outs["split"]), float((outs["pipe"] - outs["split"]).abs().max())
    assert torch.equal(outs["pipe"], outs["trace"]), float((outs["pipe"] - outs["trace"]).abs().max())


def test_split_loop_without_doubling_straddles_the_fused_ffn_limit(monkeypatch):
    """SHOW bf16 at guidance scale 1 (no doubling), B = 140: unsplit it is 12 320 rows per launch (fused FFN, hidden layer kept in fp32),
    as two sub-batch streams 6160 rows each (three launches, hidden layer rounded to bf16).  The two runs are NOT bit-identical (the
    header says so); they agree within the rows-sampled-alone gate."""
    model, cfg, sd = _handle("show", "bf16")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B, T, Cc = 140, cfg.n_poses, cfg.net_dim_pose
    audio, hub, pid = _loop_inputs(cfg, B, T, seed=29)
    keys = list(range(700, 700 + B))
    outs, fused = {}, {}
    for env in ("1", "0"):
        monkeypatch.setenv("DSH_PIPE", env)
        _lib.launch_counts(reset=True)
        outs[env] = tr.generate_batch(audio.clone(), pid.clone(), Cc, {"pretrain_aud_feat": hub.clone()}, {}, seed=13, row_keys=keys, cond_scale=1.0).clone()
        torch.cuda.synchronize()
        got = _lib.launch_counts()
        fused[env] = got["ffn_fused"]
        assert got["sample_streams"] == (1 if env == "1" else 2), got
    assert fused["1"] > 0 and fused["0"] == 0, fused
    assert torch.isfinite(outs["1"]).all()
    e = max(rel_err(outs["0"][b], outs["1"][b]) for b in range(B))
    print(f"[cond_scale 1, B=140] unsplit (fused FFN) vs two sub-batch streams (three launches): worst rel err per clip {e:.3e}, "
          f"bit-identical: {torch.equal(outs['0'], outs['1'])}")
    assert e < LOOP_TOL["bf16"]


@pytest.mark.parametrize("B", [47, 140])
def test_outpainting_window_equals_its_rows_sampled_alone(B):
    """One out-painting (masked) window — the jump schedule with the RePaint blend — above the graph range (B = 47) and above the
    two-stream limit (B = 140; a masked DDIM loop stays unsplit on the pipeline), against the rows sampled alone."""
    model, cfg, sd = _handle("show", "bf16")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    T, Cc, L = cfg.n_poses, cfg.net_dim_pose, cfg.overlap_len
    audio, hub, pid = _loop_inputs(cfg, B, T, seed=37)
    keys = list(range(2000, 2000 + B))
    gt = torch.zeros(B, T, Cc)
    gt[:, :L] = torch.randn(B, L, Cc, generator=torch.Generator().manual_seed(4))
    mask = torch.zeros(B, T, Cc, dtype=torch.bool)
    mask[:, :L] = True
    _lib.launch_counts(reset=True)
    full = tr.generate_batch(audio, pid, Cc, {"pretrain_aud_feat": hub}, {"gt": gt, "outpainting_mask": mask}, seed=21, row_keys=keys).clone()
    torch.cuda.synchronize()
    got = _lib.launch_counts()
    want = _loop_flags(B, T, "bf16", "show", True)
    assert (got["sample_graph"], got["sample_streams"]) == (want[0], want[2]), got
    assert torch.isfinite(full).all()
    worst = 0.0
    for b in _picks(B):
        y = {"gt": gt[b:b + 1], "outpainting_mask": mask[b:b + 1]}
        solo = tr.generate_batch(audio[b:b + 1], pid[b:b + 1], Cc, {"pretrain_aud_feat": hub[b:b + 1]}, y, seed=21, row_keys=[keys[b]])
        worst = max(worst, rel_err(solo[0], full[b]))
    print(f"[out-painting window B={B}] worst rel err vs the clip sampled alone: {worst:.3e}")
    assert worst < LOOP_TOL["bf16"]


def test_evaluation_does_not_depend_on_a_loop_run_before_it():
    """SHOW bf16, B = 200 (two sub-batch streams for an evaluation, one batch on the two-encoder pipeline for a loop): eval -> ddim loop ->
    eval with unchanged inputs.  The loop re-conditions the batch unsplit and set_condition keeps that shape unsplit for the NEXT loop
    (sticky shape), but an evaluation always goes back to its own split (DenoiserContext::eval: want_split unless a loop is running), so
    both evaluations report two streams; they are bit-identical and match the oracle.  A dsh_sample call that is refused after it
    began the loop must not leave the `loop running` mark behind: the evaluation after it still reports two streams."""
    from diffsheg_amd.model import UniDiffuser
    cfg, sd = get_config("show"), synthetic_sd("show")
    model = UniDiffuser(cfg, sd, device="cuda:0", precision="bf16")           # (its own context: the sticky shape must start unset)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    B, T, Cc = 200, cfg.n_poses, cfg.net_dim_pose
    inp, t, c1, c2 = _batch(cfg, B, T, 91)
    _lib.launch_counts(reset=True)
    e1 = _eval(model, "show", cfg, inp, t, c1, c2).cpu()
    s1 = _lib.launch_counts()["eval_streams"]
    x = tr.generate_batch(inp["audio_emb"].cuda(), inp["person_id"].cuda(), Cc, {"pretrain_aud_feat": inp["pretrain_aud_feat"].cuda()}, {}, seed=3)
    assert torch.isfinite(x).all() and _lib.launch_counts()["sample_pipe"] == 1
    inp2 = {k: v.clone() for k, v in inp.items()}                              # (same values, new tensors: the shim conditions again)
    e2 = _eval(model, "show", cfg, inp2, t, c1, c2).cpu()
    s2 = _lib.launch_counts()["eval_streams"]
    assert (s1, s2) == (2, 2), (s1, s2)
    assert torch.equal(e1, e2), float((e1 - e2).abs().max())
    x = tr.generate_batch(inp["audio_emb"].cuda(), inp["person_id"].cuda(), Cc, {"pretrain_aud_feat": inp["pretrain_aud_feat"].cuda()}, {}, seed=3)
    assert _lib.launch_counts()["sample_streams"] == 1                       # (conditioned as one batch: the state the refused call starts from)
    assert _refused_sample(tr, model, B, T) < 0
    e3 = _eval(model, "show", cfg, inp2, t, c1, c2).cpu()
    s3 = _lib.launch_counts()["eval_streams"]
    assert s3 == 2 and torch.equal(e1, e3), (s3, float((e1 - e3).abs().max()))
    rows = _sample_clips("bf16", B, T)
    ref = _oracle("show", sd, cfg, inp, t, c1, c2, rows)
    wm, wr = _compare("bf16", e1[torch.tensor(rows)], ref, rows, "eval-loop-eval")
    print(f"[eval -> loop -> eval, B=200] streams {s1} then {s2}, bit-identical; max|eps-ref| = {wm:.3e}, rms = {wr:.3e}")
    del tr, model
