"""precision="bf16x3" end to end on a real MI355X: the fp32 path with its large Linears on the split-bf16 main loop (gemm_f32_split.hip).

  1. one evaluation against the CPU oracle at the smallest batches that cross the few-row threshold (512 token rows), under the project's
     own bar FP32_ATOL = 1e-3 - the bar of precision="fp32";
  2. at or below the threshold the model launches the very kernels of precision="fp32": bit-identical, no split launch;
  3. a ddim25 loop stays within 1e-3 of the sample range of the fp32 loop (itself within 2e-6 of the reference by the committed goldens),
     is not bit-equal to it, and repeats bit for bit;
  4. sub-batch streams: a batch split over two streams equals the single-stream evaluation bit for bit, and sampled clips of it match the
     oracle (33 440 rows: every Linear of the model on the 128 x 128 tile, the CFG-null row constant in its epilogue included);
  5. the single-transformer model (one MotionTransformer over all 232 channels, the only `out` head wide enough for the split loop) against
     the oracle above the threshold.

The tile mixes in between, the stream splits and the few-row limit itself are walked by test_gpu_dispatch_sweep.py.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsheg_amd import _lib  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from oracle import denoiser_ref  # noqa: E402
from util import WEIGHT_SEED, eval_call, golden, gpu_model, gpu_single_model, max_abs, sample_clips, synthetic_sd  # noqa: E402

FP32_ATOL = 1e-3                      # tests/test_gpu_eval.py: the project's bar on eps


def _big_batch(cfg, B, T, seed):
    """B distinct clips with per-clip timesteps / coefficients (test_gpu_eval._big_batch)"""
    inp = make_inputs(cfg, B, frames=T, seed=seed)
    t = torch.tensor([(37 * i + 5) % 1000 for i in range(B)])
    c1 = 1.0 + 0.5 * (torch.arange(B, dtype=torch.float32) % 7) / 7
    c2 = 0.5 + 0.25 * (torch.arange(B, dtype=torch.float32) % 5) / 5
    return inp, t, c1, c2


# first, last, one straddling a 128-token boundary (BEAT: clip 3 = tokens 102 .. 135; SHOW: clip 1 = tokens 88 .. 175), two interior
@pytest.mark.parametrize("ds,B,T,rows", [("beat", 16, 34, [0, 3, 7, 11, 15]), ("show", 8, 88, [0, 1, 3, 5, 7])])
def test_evaluation_matches_the_oracle_inside_the_fp32_bar(ds, B, T, rows):
    """SHOW runs with classifier-free guidance (1 408 rows with the null half; the CFG-null row constant rides in the split launches' epilogue)."""
    cfg = get_config(ds)
    model = gpu_model(ds, "bf16x3")
    inp, t, c1, c2 = _big_batch(cfg, B, T, seed=53)
    _lib.launch_counts(reset=True)
    eps = eval_call(model, cfg, inp, t, c1, c2).cpu()
    counts = _lib.launch_counts(reset=True)
    r = torch.tensor(rows)
    with torch.no_grad():
        ref = denoiser_ref.unidiffuser(synthetic_sd(ds), cfg, inp["x_T"][r], t[r], c1[r].view(-1, 1, 1), c2[r].view(-1, 1, 1), inp["audio_emb"][r],
                                       inp["person_id"][r], inp["pretrain_aud_feat"][r])
    e = max_abs(eps[r], ref)
    e32 = max_abs(eval_call(gpu_model(ds, "fp32"), cfg, inp, t, c1, c2).cpu()[r], ref)
    print(f"[eval bf16x3 {ds} B={B} T={T}] max |eps - oracle| = {e:.3e} on clips {rows} (fp32: {e32:.3e}; |eps| max {float(ref.abs().max()):.2f}; "
          f"split launches {counts['gemm_f32_split']}, exact-fp32 gemm_f32_pro launches {counts['gemm_f32_pro']})")
    assert torch.isfinite(eps).all()
    assert e < FP32_ATOL
    assert counts["gemm_f32_split"] > 0 and counts["gemm_f32_pro"] == 0, counts


def test_single_transformer_evaluation_matches_the_oracle():
    """SHOW config, unidiffuser = False, B = 8, T = 88: 704 conditional rows, 1 408 with the null half - every layer Linear and the 232-column
    `out` head on the split loop.  Clips: first, last, clip 1 (tokens 88 .. 175 straddle a 128-row tile edge), two interior."""
    from diffsheg_amd.weights import make_synthetic_state_dict
    model = gpu_single_model("bf16x3")
    cfg = model.cfg
    sd = make_synthetic_state_dict(cfg, WEIGHT_SEED)
    B, T, rows = 8, 88, [0, 1, 3, 5, 7]
    inp, t, _, _ = _big_batch(cfg, B, T, seed=57)

    def run(m):
        return m(inp["x_T"].cuda(), t.cuda(), audio_emb=inp["audio_emb"].cuda(), length=torch.full((B,), T), person_id=inp["person_id"].cuda(),
                 add_cond={"pretrain_aud_feat": inp["pretrain_aud_feat"].cuda()}, pe_type="pe_sinu", y={}).cpu()
    _lib.launch_counts(reset=True)
    eps = run(model)
    counts = _lib.launch_counts(reset=True)
    r = torch.tensor(rows)
    with torch.no_grad():
        ref = denoiser_ref.single_motion_transformer(sd, cfg, inp["x_T"][r], t[r], inp["audio_emb"][r], inp["person_id"][r], inp["pretrain_aud_feat"][r])
    e, e32 = max_abs(eps[r], ref), max_abs(run(gpu_single_model("fp32"))[r], ref)
    print(f"[measure] eval bf16x3 single-transformer B={B} T={T}: max |eps - oracle| = {e:.3e} on clips {rows} (fp32: {e32:.3e}); "
          f"split launches {counts['gemm_f32_split']}, exact-fp32 gemm_f32_pro launches {counts['gemm_f32_pro']}")
    assert torch.isfinite(eps).all()
    assert e < FP32_ATOL
    assert counts["gemm_f32_split"] > 0 and counts["gemm_f32_pro"] == 0, counts


@pytest.mark.parametrize("ds", ["beat", "show"])
def test_below_the_few_row_threshold_it_is_the_fp32_path_bit_for_bit(ds):
    cfg = get_config(ds)
    f = golden(f"eval_{ds}.npz")
    inp = make_inputs(cfg, int(f["batch"]), seed=int(f["input_seed"]))
    args = (int(f["k14_t"]), float(f["k14_c1"]), float(f["k14_c2"]))
    a = eval_call(gpu_model(ds, "fp32"), cfg, inp, *args).clone()
    _lib.launch_counts(reset=True)
    b = eval_call(gpu_model(ds, "bf16x3"), cfg, inp, *args).clone()
    counts = _lib.launch_counts(reset=True)
    assert counts["gemm_f32_split"] == 0, counts
    assert torch.equal(a, b)
    assert max_abs(b, torch.from_numpy(f["k14_eps"])) < FP32_ATOL


def test_ddim25_stays_within_a_thousandth_of_the_range_of_the_fp32_loop():
    from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace
    cfg = get_config("beat")
    B, T = 16, 34
    inp = make_inputs(cfg, B, frames=T, seed=61)
    a, p, cnd = inp["audio_emb"].cuda(), inp["person_id"].cuda(), {"pretrain_aud_feat": inp["pretrain_aud_feat"].cuda()}
    out = {}
    for prec in ("fp32", "bf16x3"):
        tr = DDPMTrainer(sampler_namespace(cfg), gpu_model("beat", prec))
        _lib.launch_counts(reset=True)
        out[prec] = tr.generate_batch(a, p, cfg.net_dim_pose, cnd, {}, seed=4321).clone()
        c = _lib.launch_counts(reset=True)
        assert (c["gemm_f32_split"] > 0) == (prec == "bf16x3"), (prec, c)
        if prec == "bf16x3":
            again = tr.generate_batch(a, p, cfg.net_dim_pose, cnd, {}, seed=4321)
            assert torch.equal(again, out[prec]), "a repeat of the bf16x3 loop is not bit-identical"
    x32, x3 = out["fp32"].cpu().double(), out["bf16x3"].cpu().double()
    rng = float(x32.max() - x32.min())
    d = (x3 - x32).abs()
    print(f"[ddim25 beat B={B}] bf16x3 against fp32: max |d| = {float(d.max()):.3e} = {float(d.max()) / rng:.3e} of the range {rng:.2f}, "
          f"rms {float(d.pow(2).mean().sqrt()) / rng:.3e} of the range")
    assert torch.isfinite(out["bf16x3"]).all()
    assert not torch.equal(out["fp32"], out["bf16x3"])
    assert float(d.max()) < 1e-3 * rng


def test_two_stream_split_is_bit_identical(monkeypatch):
    """SHOW B = 380: 33 440 token rows, above the fp32 storage threshold of 4 096 rows, one stream (DSH_DUAL=0) against the sub-batch streams
    of the default (three at this size; test_gpu_eval.test_large_batch_two_stream_split_is_bit_identical), and sampled clips of the split
    run against the oracle: every Linear of either run is on the 128 x 128 tile."""
    from diffsheg_amd.model import UniDiffuser
    cfg = get_config("show")
    B, T = 380, 88
    inp = make_inputs(cfg, 8, frames=T, seed=5)
    rep = lambda v: v.repeat(B // 8 + 1, *([1] * (v.dim() - 1)))[:B].contiguous()
    inp = {k: rep(v) for k, v in inp.items()}
    inp["x_T"] = inp["x_T"] + 0.01 * torch.arange(B, dtype=torch.float32).view(B, 1, 1)
    t = torch.tensor([(37 * i + 5) % 1000 for i in range(B)])
    c1 = 1.0 + 0.01 * torch.arange(B, dtype=torch.float32)
    c2 = 0.5 + 0.005 * torch.arange(B, dtype=torch.float32)
    outs, streams, big = [], [], []
    for dual in ("0", "3"):
        monkeypatch.setenv("DSH_DUAL", dual)
        model = UniDiffuser(cfg, synthetic_sd("show"), device="cuda:0", precision="bf16x3")
        _lib.launch_counts(reset=True)
        outs.append(eval_call(model, cfg, inp, t, c1, c2).clone())
        c = _lib.launch_counts(reset=True)
        streams.append(c["eval_streams"])
        big.append(c["gemm_f32_split_128"])
        assert c["gemm_f32_split"] > 0 and c["gemm_f32_pro"] == 0, c
        del model
    assert streams[0] <= 1 and streams[1] >= 2, streams
    assert min(big) > 0, big
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
    # five clips against the oracle, picked as the dispatch sweep picks them (util.sample_clips): the batch ends and both sides of the
    # stream splits the run reported (fp32 storage cuts 33 440 rows into three sub-batches)
    rows = sample_clips(B, T, streams[1], cap=5)
    r = torch.tensor(rows)
    with torch.no_grad():
        ref = denoiser_ref.unidiffuser(synthetic_sd("show"), cfg, inp["x_T"][r], t[r], c1[r].view(-1, 1, 1), c2[r].view(-1, 1, 1), inp["audio_emb"][r],
                                       inp["person_id"][r], inp["pretrain_aud_feat"][r])
    e = max_abs(outs[1].cpu()[r], ref)
    print(f"[measure] eval bf16x3 show B={B} T={T}, {streams[1]} streams, 128 x 128 launches {big}: max |eps - oracle| = {e:.3e} on clips {rows}")
    assert e < FP32_ATOL
