"""Clips of different lengths in one batch on a real MI355X (dsh_set_condition_ragged): the length-aware attention kernels at op
level, evaluations of padded batches against the CPU oracle run on every clip ALONE at its own length, independence of whatever the
padded frames hold, bit-identity of the no-lengths paths, sampling loops and chains against the clip / chain sampled alone, and the
refusals.  Gates are the project's existing ones for the same comparisons: evaluation fp32 1e-3 abs, bf16 max
6e-2 / rms 1.5e-2 (tests/test_gpu_eval.py); loops and chains vs the row alone fp32 1e-5 of range, bf16 1.2e-2
(tests/test_gpu_sharded.py); attention cores fp32 1e-3 abs, bf16 2e-2 max(1, |ref|) (tests/test_gpu_ops.py)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsheg_amd import _lib  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace, seam_windows, split_segments, split_segments_for_repair  # noqa: E402
from oracle import denoiser_ref  # noqa: E402
from ragged_util import GARBAGE, attention_ref  # noqa: E402
from diffsheg_amd.weights import make_synthetic_state_dict  # noqa: E402
from util import F32_STORAGE, WEIGHT_SEED, assert_split_ran, gpu_model, gpu_single_model, oracle_ddim25, philox_rows, rel_err, synthetic_sd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_ATOL, BF16_MAX, BF16_RMS = 1e-3, 6e-2, 1.5e-2
LOOP_FP32, LOOP_BF16 = 1e-5, 1.2e-2
DEV = "cuda:0"


def _p(t):
    return C.c_void_p(t.data_ptr())


def _lens_for(B, T):
    """Mixed lengths for a batch padded to T frames: the full length, one frame, tile edges of the attention kernels (12 k, 32, 33),
    T - 1 and a few in between.  The first clip is short, so a batch of one is a padded clip too."""
    pat = [max(1, (7 * T) // 10), T, max(1, (2 * T) // 9), 4, T - 1, 33, 32, 12, 1, 24, (T + 1) // 2]
    return [min(T, max(1, pat[b % len(pat)])) for b in range(B)]


def _batch(cfg, B, T, seed):
    small = make_inputs(cfg, min(B, 64), frames=T, seed=seed)
    rep = (B + 63) // 64
    out = {k: v.repeat(*([rep] + [1] * (v.dim() - 1)))[:B].clone() for k, v in small.items()}
    if B > 64:                                             # (repeated rows differ a little: no two clips of a big batch are equal)
        g = torch.Generator().manual_seed(seed + 1)
        out["audio_emb"] += 0.01 * torch.randn(out["audio_emb"].shape, generator=g)
        out["x_T"] += 0.01 * torch.randn(out["x_T"].shape, generator=g)
    pid = torch.zeros(B, cfg.style_dim)
    pid[torch.arange(B), torch.arange(B) % cfg.style_dim] = 1.0
    out["person_id"] = pid
    return out


def _fill_pads(inp, lens, fill):
    out = {k: v.clone() for k, v in inp.items()}
    for b, n in enumerate(lens):
        for k in ("audio_emb", "pretrain_aud_feat", "x_T"):
            out[k][b, n:] = fill if k != "pretrain_aud_feat" else -fill
    return out


def _eval(model, cfg, inp, t, c1, c2, lengths, single=False):
    B, T = inp["x_T"].shape[:2]
    kw = dict(audio_emb=inp["audio_emb"].cuda(), length=None if lengths is None else torch.tensor(lengths), person_id=inp["person_id"].cuda(),
              add_cond={"pretrain_aud_feat": inp["pretrain_aud_feat"].cuda()}, pe_type="pe_sinu", y={})
    if single:
        return model(inp["x_T"].cuda(), t.cuda(), **kw)
    shape_e = (B, T, cfg.expression_dim)
    sa = [c1.view(B, 1, 1).expand(shape_e), c2.view(B, 1, 1).expand(shape_e)]
    return model(inp["x_T"].cuda(), t.cuda(), sqrt_alphas=sa, **kw)


@functools.lru_cache(maxsize=2)
def _single_sd(ds):
    return make_synthetic_state_dict(get_config(ds, unidiffuser=False), WEIGHT_SEED)


def _oracle_alone(ds, cfg_o, inp, b, n, t, c1, c2, single):
    sd = _single_sd(ds) if single else synthetic_sd(ds)
    with torch.no_grad():
        if single:
            return denoiser_ref.single_motion_transformer(sd, cfg_o, inp["x_T"][b:b + 1, :n], t[b:b + 1], inp["audio_emb"][b:b + 1, :n],
                                                          inp["person_id"][b:b + 1], inp["pretrain_aud_feat"][b:b + 1, :n])[0]
        return denoiser_ref.unidiffuser(sd, cfg_o, inp["x_T"][b:b + 1, :n], t[b:b + 1], c1[b].view(1, 1, 1), c2[b].view(1, 1, 1),
                                        inp["audio_emb"][b:b + 1, :n], inp["person_id"][b:b + 1], inp["pretrain_aud_feat"][b:b + 1, :n])[0]


# ---- 4. the six attention kernels, each reached by the shape that selects it --------------------------------------------------
from bf16_gates import attn_lens as _attn_lens  # noqa: E402  (shared with test_gpu_bf16_attention_families.py and the CPU proof of its gates)


# (name, dtype, variant, D, head_dim, T): fp32 MFMA kernel at each of its four tile sizes; the pre-loaded VALU kernel (encoder_aud, hd 16);
# the loop kernel (> 96 frames) at both head widths; the fp32 kernel with the StylizationBlock front; bf16: tiled MFMA (whole-chip and
# window-chain batches take this one), row-major MFMA, pre-loaded and loop kernels
ATTN_CASES = [("f32_mfma", 0, 0, 512, 64, 32), ("f32_mfma", 0, 0, 512, 64, 34), ("f32_mfma", 0, 0, 512, 64, 64), ("f32_mfma", 0, 0, 512, 64, 88),
              ("pre", 0, 0, 128, 16, 88), ("pre", 0, 0, 128, 16, 34), ("loop", 0, 0, 128, 16, 120), ("loop", 0, 0, 512, 64, 120),
              ("sty", 0, 2, 512, 64, 30), ("sty", 0, 2, 512, 64, 34), ("sty", 0, 2, 512, 64, 64),
              ("tiled", 1, 0, 512, 64, 88), ("tiled", 1, 0, 512, 64, 34), ("tiled", 1, 0, 512, 64, 96), ("mfma_bf16", 1, 1, 512, 64, 88),
              ("pre", 1, 1, 128, 16, 88), ("loop", 1, 1, 512, 64, 120), ("loop", 1, 1, 128, 16, 120)]


@pytest.mark.parametrize("doubled", [False, True])
@pytest.mark.parametrize("name,dtype,variant,D,hd,T", ATTN_CASES)
def test_attention_kernels_exclude_padded_frames(name, dtype, variant, D, hd, T, doubled):
    """K / V rows of padded frames hold NaN and +-inf: exclusion is by selection, so valid AND padded query rows stay finite and the
    valid ones equal the fp64 expression on the clip's own frames.  `doubled`: a CFG-doubled batch, both halves share the lengths."""
    lens = _attn_lens(T)
    nl = len(lens)
    nb = 2 * nl if doubled else nl
    g = torch.Generator().manual_seed(1000 * T + D + nb)
    qkv = torch.randn(nb, T, 3 * D, generator=g) * 2
    tdt = torch.bfloat16 if dtype else torch.float32
    qkv = qkv.to(tdt)
    ref = attention_ref(qkv, lens, hd)                       # (on the values the kernel reads)
    bad = qkv.clone()
    for b in range(nb):
        n = lens[b % nl]
        bad[b, n:, D:2 * D] = float("nan") if b % 2 else float("inf")
        bad[b, n:, 2 * D:] = float("-inf") if b % 2 else float("nan")
    L = _lib.lib()
    qd, ld = bad.to(DEV).contiguous(), torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = torch.full((nb, T, D), float("nan"), device=DEV, dtype=tdt)
    film = None
    if variant == 2:
        film = torch.randn(nl, 2 * D, generator=g).to(DEV).contiguous()
        y = ref
        xh = (y - y.mean(-1, keepdim=True)) / torch.sqrt(y.var(-1, unbiased=False, keepdim=True) + 1e-5)
        fl = film.cpu().double().repeat(nb // nl, 1)
        ref = torch.nn.functional.silu(xh * fl[:, None, :D] + fl[:, None, D:])
    _lib.check(L.dsh_op_linear_attention_ragged(None, dtype, variant, _p(qd), nb, T, D, hd, _p(out), _p(ld), nl, None if film is None else _p(film)))
    torch.cuda.synchronize()
    o = out.cpu().double()
    assert torch.isfinite(o).all(), "a padded K / V value reached an output"
    worst = max(float((o[b, :lens[b % nl]] - ref[b, :lens[b % nl]]).abs().max()) for b in range(nb))
    gate = 2e-2 * max(1.0, float(ref.abs().max())) if dtype else 1e-3
    print(f"[ragged attention {name} dtype {dtype} D {D} hd {hd} T {T} nb {nb}] worst |y - ref| on valid frames {worst:.3e} (gate {gate:.1e})")
    assert worst < gate
    # no lengths, and lengths all = T: the plain launch, bit for bit
    if variant != 2:
        clean = qkv.to(DEV).contiguous()
        plain, viaragged, full = (torch.empty(nb, T, D, device=DEV, dtype=tdt) for _ in range(3))
        if dtype == 0:
            _lib.check(L.dsh_op_linear_attention(None, _p(clean), nb, T, D, hd, _p(plain)))
        elif variant == 0:
            _lib.check(L.dsh_op_linear_attention_bf16(None, _p(clean), nb, T, D, hd, _p(plain)))
        else:
            _lib.check(L.dsh_op_linear_attention_ragged(None, dtype, variant, _p(clean), nb, T, D, hd, _p(plain), None, 0, None))
        _lib.check(L.dsh_op_linear_attention_ragged(None, dtype, variant, _p(clean), nb, T, D, hd, _p(viaragged), None, 0, None))
        lt = torch.full((nl,), T, dtype=torch.int32, device=DEV)
        _lib.check(L.dsh_op_linear_attention_ragged(None, dtype, variant, _p(clean), nb, T, D, hd, _p(full), _p(lt), nl, None))
        torch.cuda.synchronize()
        assert torch.equal(plain, viaragged)
        # (bf16 tiled: the existing entry splits the batch into other halves; the values are the same)
        assert torch.equal(plain, full), float((plain.float() - full.float()).abs().max())


# ---- 5 / 6. evaluation of padded batches -----------------------------------------------------------------------------------------
def _picks(B):
    if B <= 11:
        return list(range(B))
    return sorted({0, 1, 2, 3, B // 3 - 1, B // 3, B // 3 + 1, B // 2 - 1, B // 2, B // 2 + 1, 2 * B // 3 - 1, 2 * B // 3, 2 * B // 3 + 1, B - 3, B - 2, B - 1})


def _check_eval(ds, precision, B, T, cfg_on=True, single=False, seed=40):
    cfg = get_config(ds, unidiffuser=False) if single else get_config(ds)
    cfg_o = cfg if cfg_on else (get_config(ds, unidiffuser=False, cond_scale=1.0) if single else get_config(ds, cond_scale=1.0))
    model = gpu_single_model(precision, ds) if single else gpu_model(ds, precision)
    lens = _lens_for(B, T)
    if precision == "bf16x3" and 1 not in lens:
        lens[2] = 1                                        # a clip of ONE frame beside full ones: T - 1 all-zero rows through the PRO 1 row shift
    inp = _batch(cfg, B, T, seed + B)
    t = torch.full((B,), 520, dtype=torch.long)
    c1, c2 = torch.full((B,), 1.7), torch.full((B,), 1.3)
    prev = model.guidance_scale
    if not cfg_on:
        model.set_guidance_scale(1.0)
    try:
        _lib.launch_counts(reset=True)
        out = _eval(model, cfg, _fill_pads(inp, lens, 0.0), t, c1, c2, lens, single).cpu()
        counts = _lib.launch_counts()
        out_g = _eval(model, cfg, _fill_pads(inp, lens, GARBAGE), t, c1, c2, lens, single).cpu()
    finally:
        if not cfg_on:
            model.set_guidance_scale(prev)
    assert model.lengths == tuple(lens)
    assert torch.isfinite(out).all() and torch.isfinite(out_g).all()
    # 6. whatever the padded frames of x, mel and HuBERT hold: valid frames bit-identical
    for b, n in enumerate(lens):
        assert torch.equal(out[b, :n], out_g[b, :n]), (b, n, float((out[b, :n] - out_g[b, :n]).abs().max()))
    # 5. rows vs the ORACLE on the clip alone at T = its length
    worst, sq, cnt = 0.0, 0.0, 0
    for b in _picks(B):
        n = lens[b]
        ref = _oracle_alone(ds, cfg_o, inp, b, n, t, c1, c2, single)
        d = (out[b, :n] - ref).double()
        worst = max(worst, float(d.abs().max()))
        sq += float((d * d).sum())
        cnt += d.numel()
    rms = (sq / cnt) ** 0.5
    print(f"[ragged eval {ds} {precision} B={B} T={T} cfg={'on' if cfg_on else 'off'} single={single}] lengths {sorted(set(lens))}: "
          f"{len(_picks(B))} clips vs the oracle alone: max {worst:.3e} rms {rms:.3e}")
    if precision == "bf16x3":
        # (above 512 rows: the split loop ran; the fp32 path's distance on the same batch is printed beside it)
        assert B * T > 512
        assert_split_ran(counts, (ds, B, T))
        o32 = _eval(gpu_single_model("fp32", ds) if single else gpu_model(ds, "fp32"), cfg, _fill_pads(inp, lens, 0.0), t, c1, c2, lens, single).cpu()
        w32 = max(float((o32[b, :lens[b]] - _oracle_alone(ds, cfg_o, inp, b, lens[b], t, c1, c2, single)).abs().max()) for b in _picks(B)[:4])
        print(f"[measure] ragged eval {ds} bf16x3 B={B} T={T}: max |eps - oracle| {worst:.3e} (fp32 on the first four of these clips: {w32:.3e}); "
              f"split launches {counts['gemm_f32_split']}")
    if precision in F32_STORAGE:
        assert worst < FP32_ATOL
    else:
        assert worst < BF16_MAX and rms < BF16_RMS


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("B", list(range(1, 12)))
def test_ragged_eval_window_chain_batches_show(precision, B):
    _check_eval("show", precision, B, 88)


@pytest.mark.parametrize("ds,precision,B,T,cfg_on,single", [
    ("show", "fp32", 5, 88, False, False), ("show", "bf16", 5, 88, False, False),          # guidance scale 1: no doubled batch
    ("beat", "fp32", 1, 34, True, False), ("beat", "fp32", 7, 34, True, False), ("beat", "fp32", 11, 34, True, False),
    ("show", "fp32", 6, 88, True, True), ("show", "bf16", 6, 88, True, True),              # the single MotionTransformer
    ("show", "fp32", 9, 30, True, False), ("show", "bf16", 9, 30, True, False),            # a tail window as the padded shape
    ("show", "fp32", 100, 88, True, False), ("show", "bf16", 100, 88, True, False),        # mid-size (fp32: two sub-batch streams)
    ("show", "bf16", 950, 88, True, False), ("beat", "fp32", 256, 34, True, False),        # the headline batches: three sub-batch streams
    ("beat", "bf16x3", 16, 34, True, False), ("show", "bf16x3", 6, 88, True, False)])      # the split-bf16 loop: the smallest batches above 512 rows
def test_ragged_eval_other_regimes(ds, precision, B, T, cfg_on, single):
    _check_eval(ds, precision, B, T, cfg_on, single)


# ---- 7 / 10. the native entry: all-full lengths, refusals ------------------------------------------------------------------------
def _raw(model, cfg, inp, t, c1, c2, lens):
    """dsh_set_condition[_ragged] + dsh_eval straight through the C ABI (the Python layer turns all-full lengths into no lengths)."""
    L = _lib.lib()
    B, T = inp["x_T"].shape[:2]
    a, p, h, x = (inp[k].to(DEV).contiguous() for k in ("audio_emb", "person_id", "pretrain_aud_feat", "x_T"))
    td, c1d, c2d = t.to(DEV), c1.to(DEV), c2.to(DEV)
    out = torch.empty_like(x)
    model._cond_key = None
    if lens is None:
        rc = L.dsh_set_condition(model._h, B, T, _p(a), _p(p), _p(h))
    else:
        rc = L.dsh_set_condition_ragged(model._h, B, T, (C.c_int32 * B)(*lens), _p(a), _p(p), _p(h))
    if rc != 0:
        return rc, None, None
    _lib.launch_counts(reset=True)
    _lib.check(L.dsh_eval(model._h, _p(x), _p(td), _p(c1d), _p(c2d), _p(out)), "dsh_eval")
    torch.cuda.synchronize()
    return 0, out.cpu(), _lib.launch_counts()


@pytest.mark.parametrize("ds,precision,B", [("show", "fp32", 3), ("show", "bf16", 3), ("show", "bf16", 950), ("beat", "fp32", 256), ("show", "fp32", 100)])
def test_all_full_lengths_are_the_plain_path_and_refusals_keep_the_condition(ds, precision, B):
    cfg = get_config(ds)
    model = gpu_model(ds, precision)
    T = cfg.n_poses
    inp = _batch(cfg, B, T, 70 + B)
    t = torch.full((B,), 300, dtype=torch.long)
    c1, c2 = torch.full((B,), 1.4), torch.full((B,), 0.9)
    rc, plain, n_plain = _raw(model, cfg, inp, t, c1, c2, None)
    assert rc == 0
    rc, full, n_full = _raw(model, cfg, inp, t, c1, c2, [T] * B)
    assert rc == 0 and torch.equal(plain, full), float((plain - full).abs().max())
    assert n_plain == n_full, (n_plain, n_full)
    # a ragged condition in between leaves nothing behind: dsh_set_condition clears the lengths
    lens = _lens_for(B, T)
    rc, rag, n_rag = _raw(model, cfg, inp, t, c1, c2, lens)
    assert rc == 0 and n_rag == n_plain and not torch.equal(rag, plain)
    rc, again, _ = _raw(model, cfg, inp, t, c1, c2, None)
    assert rc == 0 and torch.equal(again, plain)
    # 10. refused before any state changes: -1, and the previous condition still evaluates to the same bits
    L = _lib.lib()
    for bad in ([0] + [T] * (B - 1), [T] * (B - 1) + [T + 1], [-3] + [T] * (B - 1)):
        rc, _, _ = _raw(model, cfg, inp, t, c1, c2, bad)
        assert rc == -1 and b"length" in L.dsh_last_error()
        x, td, c1d, c2d = inp["x_T"].to(DEV).contiguous(), t.to(DEV), c1.to(DEV), c2.to(DEV)
        out = torch.empty_like(x)
        _lib.check(L.dsh_eval(model._h, _p(x), _p(td), _p(c1d), _p(c2d), _p(out)), "dsh_eval")
        assert torch.equal(out.cpu(), plain)
    model._cond_key = None


def test_python_refusals():
    cfg = get_config("show")
    model = gpu_model("show", "fp32")
    B, T = 3, 40
    inp = _batch(cfg, B, T, 5)
    lens = [40, 22, 7]
    a, p, h = inp["audio_emb"].cuda(), inp["person_id"].cuda(), inp["pretrain_aud_feat"].cuda()
    for bad in ([40, 0, 7], [41, 22, 7], [40, 22]):
        with pytest.raises(ValueError):
            model.set_condition(a, p, h, lengths=bad)
    tr = DDPMTrainer(sampler_namespace(cfg, same_overlap_noisy=True), model)
    with pytest.raises(NotImplementedError):
        tr.generate_batch(a, p, cfg.net_dim_pose, {"pretrain_aud_feat": h}, {}, seed=1, lengths=lens)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    y = {"gt": torch.zeros(B, T, cfg.net_dim_pose), "outpainting_mask": torch.ones(B, T, cfg.net_dim_pose, dtype=torch.bool), "outpainting_mask_any": True}
    with pytest.raises(NotImplementedError):
        tr.generate_batch(a, p, cfg.net_dim_pose, {"pretrain_aud_feat": h}, y, seed=1, lengths=lens, tail_blend=True)
    # the native loop refuses the combination itself (-1), whoever calls it
    model.set_condition(a, p, h, lengths=lens)
    model._cond_key = None
    L = _lib.lib()
    opts = tr.diffusion_ddim_val._opts(0, False, 1, 5)
    x = torch.zeros(B, T, cfg.net_dim_pose, device=DEV)
    _lib.check(L.dsh_sample_set_tail_blend(model._h, 1))
    try:
        assert L.dsh_sample(model._h, C.byref(opts), _p(x), 0, None, None, 0, None, 0, None) == -1
    finally:
        L.dsh_sample_set_tail_blend(model._h, 0)
    opts.same_overlap_noisy = 1
    assert L.dsh_sample(model._h, C.byref(opts), _p(x), 0, None, None, 0, None, 0, None) == -1
    # ... and still samples the ragged condition afterwards
    out = tr.generate_batch(a, p, cfg.net_dim_pose, {"pretrain_aud_feat": h}, {}, seed=1, lengths=lens)
    assert torch.isfinite(out).all() and float(out[1, 22:].abs().max()) == 0.0 and float(out[2, 7:].abs().max()) == 0.0


# ---- 8. loops with row keys: every row vs the same clip sampled alone with its key ------------------------------------------------
def _loop_case(ds, precision, B, T, kind, expect):
    cfg = get_config(ds)
    model = gpu_model(ds, precision)
    Cc, L = cfg.net_dim_pose, cfg.overlap_len
    over = {"ddim": False, "diffusion_steps": 50} if kind == "ddpm50" else {}
    tr = DDPMTrainer(sampler_namespace(cfg, **over), model)
    lens = [max(n, L + 1) for n in _lens_for(B, T)] if kind == "outpaint" else _lens_for(B, T)
    inp = _fill_pads(_batch(cfg, B, T, 90 + B), lens, GARBAGE)
    a, p, h = inp["audio_emb"].cuda(), inp["person_id"].cuda(), inp["pretrain_aud_feat"].cuda()
    keys = [5000 + 7 * b for b in range(B)]
    kw = {"eta": 0.5} if kind == "eta" else {}

    def y_for(rows, frames):
        if kind != "outpaint":
            return {}
        g = torch.Generator().manual_seed(3)
        gt_all = torch.randn(B, L, Cc, generator=g)
        gt = torch.zeros(len(rows), frames, Cc, device=DEV)
        gt[:, :L] = gt_all[rows].to(DEV)
        mask = torch.zeros(len(rows), frames, Cc, dtype=torch.bool, device=DEV)
        mask[:, :L] = True
        return {"gt": gt, "outpainting_mask": mask, "outpainting_mask_any": True}
    _lib.launch_counts(reset=True)
    full = tr.generate_batch(a, p, Cc, {"pretrain_aud_feat": h}, y_for(list(range(B)), T), seed=77, row_keys=keys, lengths=lens, **kw)
    torch.cuda.synchronize()
    got = _lib.launch_counts()
    regime = {k: got[k] for k in ("sample_streams", "sample_graph", "sample_pipe")}
    assert full.shape == (B, T, Cc) and torch.isfinite(full).all()
    for k, v in expect.items():
        assert regime[k] == v, (regime, expect)
    worst = 0.0
    for b in _picks(B):
        n = lens[b]
        assert float(full[b, n:].abs().max()) == 0.0 if n < T else True
        solo = tr.generate_batch(a[b:b + 1, :n].contiguous(), p[b:b + 1], Cc, {"pretrain_aud_feat": h[b:b + 1, :n].contiguous()}, y_for([b], n),
                                 seed=77, row_keys=[keys[b]], **kw)
        worst = max(worst, rel_err(full[b, :n], solo[0]))
    for b, n in enumerate(lens):
        if n < T:
            assert float(full[b, n:].abs().max()) == 0.0
    if precision == "bf16x3":
        # A clip alone is below 512 rows and runs the fp32 kernels: the comparison above crosses a change of arithmetic, so it is a
        # measurement here.  The 1e-5 gate is held by the same clips inside ANOTHER batch that is above 512 rows as well (four more clips
        # behind them: other tiles, other sub-batch boundaries), and the loop itself by the oracle's loop on two clips under 1e-3.
        assert B * T > 512 and kind == "ddim25"
        assert_split_ran(got, (ds, B))
        print(f"[measure] ragged loop {ds} bf16x3 B={B}: batch against the clip sampled alone (fp32 kernels): worst rel err {worst:.3e} (no gate)")
        cat = lambda v: torch.cat([v, v[:4]]).contiguous()
        other = tr.generate_batch(cat(a), cat(p), Cc, {"pretrain_aud_feat": cat(h)}, {}, seed=77, row_keys=keys + [9001, 9002, 9003, 9004], lengths=lens + lens[:4])
        w2 = max(rel_err(other[b, :lens[b]], full[b, :lens[b]]) for b in range(B))
        print(f"[ragged loop {ds} bf16x3] the {B} clips inside a batch of {B + 4}: worst rel err {w2:.3e} (gate {LOOP_FP32:.1e})")
        assert w2 < LOOP_FP32
        sd = synthetic_sd(ds)
        for b in (1, 0):                                     # a full clip and a short one (lengths T and 7 T / 10)
            n = lens[b]
            xT = philox_rows(77, [keys[b]], T * Cc).view(1, T, Cc)[:, :n]
            xr = oracle_ddim25(sd, cfg, inp["audio_emb"][b:b + 1, :n], inp["pretrain_aud_feat"][b:b + 1, :n], inp["person_id"][b:b + 1], xT)
            eo = rel_err(full[b, :n], xr[0])
            print(f"[measure] ragged loop {ds} bf16x3 B={B}: clip {b} ({n} frames) vs the oracle's 25-step loop from the same x_T: {eo:.3e} of the range")
            assert eo < 1e-3
        return
    tol = LOOP_FP32 if precision == "fp32" else LOOP_BF16
    print(f"[ragged loop {kind} {ds} {precision} B={B}] regime {regime}; {len(_picks(B))} rows vs the clip sampled alone: worst rel err {worst:.3e} (gate {tol:.1e})")
    assert worst < tol


SMALL_LOOPS = [(ds, precision, kind) for ds, precision in (("show", "fp32"), ("show", "bf16"), ("beat", "fp32")) for kind in ("ddim25", "outpaint", "eta", "ddpm50")]
SMALL_LOOPS.append(("beat", "bf16x3", "ddim25"))             # B = 16 (544 rows): the smallest batch on the split-bf16 loop


@pytest.mark.parametrize("ds,precision,kind", SMALL_LOOPS, ids=lambda v: str(v))
def test_ragged_loops_small_batch(ds, precision, kind):
    """Graph range (B x T_pad <= 4096 token rows): captured graphs; UniDiffuser loops run the two-encoder pipeline."""
    _loop_case(ds, precision, 16 if precision == "bf16x3" else 9, get_config(ds).n_poses, kind, {"sample_streams": 1, "sample_graph": 1})


@pytest.mark.parametrize("ds,precision,B", [("show", "bf16", 100), ("beat", "fp32", 256)])
def test_ragged_loop_pipelined_regime(ds, precision, B):
    """Above the graph range, below the sub-batch split: one batch, the two encoders' chains on two streams."""
    _loop_case(ds, precision, B, get_config(ds).n_poses, "ddim25", {"sample_streams": 1, "sample_graph": 0, "sample_pipe": 1})


@pytest.mark.parametrize("ds,precision,B,pipe_env", [("show", "bf16", 950, "1"), ("beat", "fp32", 256, "0"), ("beat", "bf16x3", 256, "0")])
def test_ragged_loop_sub_batch_streams(ds, precision, B, pipe_env, monkeypatch):
    """The headline batches on three sub-batch streams (BEAT fp32 B = 256 with DSH_PIPE=0, which is where it splits): every stream runs the
    whole loop on its slice of the clips, of the lengths and of the row keys."""
    monkeypatch.setenv("DSH_PIPE", pipe_env)
    _loop_case(ds, precision, B, get_config(ds).n_poses, "ddim25", {"sample_streams": 3, "sample_pipe": 0})


# ---- 9. chains ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ragged_chains_equal_the_chains_alone(precision):
    """Chains that end in different windows and with different tails, sampled together: every chain vs the chain alone."""
    cfg = get_config("show")
    model = gpu_model("show", precision)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    step = cfg.n_poses - cfg.overlap_len
    lens = [3 * step + 10, 2 * step + 10 + 11, 88, 40, 3 * step + 10 + 37, step + 10 + 1, 2 * step + 10]
    N = max(lens)
    inp = make_inputs(cfg, len(lens), frames=N, seed=23)
    a, h, p = inp["audio_emb"].cuda(), inp["pretrain_aud_feat"].cuda(), inp["person_id"].cuda()
    for b, n in enumerate(lens):
        a[b, n:] = GARBAGE
        h[b, n:] = -GARBAGE
    keys = [40 + b for b in range(len(lens))]
    outs = tr.sample_arbitrary_len(a, p, {"pretrain_aud_feat": h}, seed=31, row_keys=keys, lengths=lens)
    tol = LOOP_FP32 if precision == "fp32" else LOOP_BF16
    worst = 0.0
    for b, n in enumerate(lens):
        assert tuple(outs[b].shape) == (n, cfg.net_dim_pose) and torch.isfinite(outs[b]).all()
        solo = tr.sample_arbitrary_len(a[b:b + 1, :n].contiguous(), p[b:b + 1], {"pretrain_aud_feat": h[b:b + 1, :n].contiguous()}, seed=31, row_keys=[keys[b]])
        worst = max(worst, rel_err(outs[b], solo[0]))
    print(f"[ragged chains {precision}] {len(lens)} chains of {lens} frames vs each alone: worst rel err {worst:.3e} (gate {tol:.1e})")
    assert worst < tol


@pytest.mark.parametrize("N,n_seg,precision", [(1000, 5, "fp32"), (1000, 5, "bf16"), (9000, 32, "bf16")])
def test_ragged_sharded_stream_equals_its_chains_alone(N, n_seg, precision):
    cfg = get_config("show")
    model = gpu_model("show", precision)
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    inp = make_inputs(cfg, 1, frames=N, seed=15)
    audio, cond, pid = inp["audio_emb"].cuda(), {"pretrain_aud_feat": inp["pretrain_aud_feat"].cuda()}, inp["person_id"].cuda()
    out = tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=31, ragged=True)
    assert out.shape == (1, N, cfg.net_dim_pose) and torch.isfinite(out).all()
    segs = split_segments(N, n_seg, cfg.n_poses, cfg.overlap_len)
    assert len({len(s) for s in segs}) > 1                   # (otherwise nothing is ragged)
    tol = LOOP_FP32 if precision == "fp32" else LOOP_BF16
    worst = 0.0
    for i, sg in enumerate(segs):
        solo = tr.sample_arbitrary_len(audio[:, sg.start:sg.stop].contiguous(), pid, {k: v[:, sg.start:sg.stop].contiguous() for k, v in cond.items()},
                                       seed=31, row_keys=[i])
        worst = max(worst, rel_err(out[0, sg.start:sg.stop], solo[0]))
    print(f"[ragged sharded {precision} {N} frames / {len(segs)} chains of {sorted({len(s) for s in segs})} frames] worst rel err vs the chain alone {worst:.3e} (gate {tol:.1e})")
    assert worst < tol
    if N == 1000:
        # seam repair runs behind the ragged chains: frames outside the seam windows are the un-repaired ragged stream, bit for bit
        rep = tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=31, ragged=True, seam_repair=True)
        segs_r = split_segments_for_repair(N, n_seg, cfg.n_poses, cfg.overlap_len)
        assert len(segs_r) == len(segs)
        keep = torch.ones(N, dtype=torch.bool)
        for w in seam_windows(segs_r, cfg.n_poses):
            keep[w.start:w.stop] = False
        assert torch.equal(rep[:, keep], out[:, keep]) and not torch.equal(rep, out)


def _free_port():
    import socket
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


def test_ragged_sharding_through_rccl_at_world_size_1():
    """The ragged stream through the per-rank code paths (broadcast, shard, device-side gather over RCCL) as a process group of one rank
    (DSH_FORCE_COLLECTIVES=1) equals the non-collective call bit for bit."""
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rccl_ragged_world1_worker.py")], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "RCCL_RAGGED_WORLD1_OK" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2500:])
