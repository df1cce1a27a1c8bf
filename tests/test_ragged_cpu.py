"""CPU tests (-m "not gpu") of clips of different lengths in one batch: the window plan of ragged chains, chain assembly and
`ragged=True` sharding through a stub sampler (world 2 == world 1), and the oracle property the native kernels implement — a padded
evaluation with the three masks equals every clip evaluated alone."""
import inspect
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from diffsheg_amd.config import get_config
from ragged_util import clips_alone, masked_oracle, pad_batch, person_ids, stream_inputs, stub_trainer
from util import synthetic_sd

torch.set_num_threads(min(8, os.cpu_count() or 1))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. window plan ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_poses,L", [(88, 10), (34, 4)])
def test_window_plan_gives_every_chain_its_own_windows(n_poses, L):
    from diffsheg_amd.trainer import get_windows, ragged_window_plan, window_lengths
    step = n_poses - L
    # short streams (N <= n_poses), exact multiples of the stride (+ overlap), tails of overlap_len + 1 frames, everything around them
    ns = sorted(set([1, 2, L, L + 1, n_poses - 1, n_poses, n_poses + 1] + [k * step + L + d for k in range(1, 6) for d in (-1, 0, 1, 2, step // 2)]
                    + list(range(3 * step, 3 * step + 25))))
    for n in ns:
        x = torch.arange(n).view(1, n, 1)
        alone = get_windows(x, n_poses, step)
        assert [w.shape[1] for w in alone] == window_lengths(n, n_poses, step), n
    plan = ragged_window_plan(ns, n_poses, step)
    for b, n in enumerate(ns):
        x = torch.arange(n).view(1, n, 1)
        alone = get_windows(x, n_poses, step)
        mine = [(wb["start"], wb["lengths"][wb["rows"].index(b)], wb["frames"]) for wb in plan if b in wb["rows"]]
        assert len(mine) == len(alone), n
        for (start, ln, pad), w in zip(mine, alone):
            assert torch.equal(x[:, start:start + ln], w) and ln <= pad, n
    for i, wb in enumerate(plan):
        assert wb["start"] == i * step and wb["frames"] >= max(wb["lengths"])
        assert wb["frames"] == max(wb["lengths"]) or (len(wb["rows"]) >= 7 and wb["frames"] == 11)
    # a batch of seven short tails is padded to the 11 frames bf16 batches of 7 and more clips need
    assert ragged_window_plan([5] * 7, n_poses, step)[0]["frames"] == 11
    assert ragged_window_plan([5] * 6, n_poses, step)[0]["frames"] == 5


# ---- 2. chain assembly and sharding with a stub sampler ------------------------------------------------------------------------
def _alone(tr, audio, cond, pid, rng, key, seed, **kw):
    return tr.sample_arbitrary_len(audio[:, rng.start:rng.stop], pid, {k: v[:, rng.start:rng.stop] for k, v in cond.items()},
                                   seed=seed, row_keys=[key], **kw)[0]


@pytest.mark.parametrize("ds", ["show", "beat"])
def test_ragged_chains_equal_the_chains_alone(ds):
    cfg = get_config(ds)
    n_poses, L = cfg.n_poses, cfg.overlap_len
    step = n_poses - L
    lens = [3 * step + L, 5, n_poses, 2 * step + L + 1, 4 * step + L + step // 2, n_poses + 1, 2 * step + L, 3 * step + L + 7]
    N = max(lens)
    g = torch.Generator().manual_seed(2)
    audio = torch.randn(len(lens), N, cfg.audio_dim, generator=g)
    cond = {"pretrain_aud_feat": torch.randn(len(lens), N, 16, generator=g)}
    pid = torch.eye(cfg.style_dim)[torch.arange(len(lens)) % cfg.style_dim]
    keys = [100 + 3 * b for b in range(len(lens))]
    calls = []
    tr = stub_trainer(cfg, calls)
    outs = tr.sample_arbitrary_len(audio, pid, cond, seed=7, row_keys=keys, lengths=lens)
    assert isinstance(outs, list) and [tuple(o.shape) for o in outs] == [(n, cfg.net_dim_pose) for n in lens]
    one = stub_trainer(cfg)
    for b, n in enumerate(lens):
        want = one.sample_arbitrary_len(audio[b:b + 1, :n], pid[b:b + 1], {k: v[b:b + 1, :n] for k, v in cond.items()}, seed=7, row_keys=[keys[b]])[0]
        assert torch.equal(outs[b], want), (b, n)
    # window i holds the chains that have a window i; equal rows go without lengths (the path it always was)
    from diffsheg_amd.trainer import window_lengths
    assert [c["B"] for c in calls] == [sum(1 for n in lens if len(window_lengths(n, n_poses, step)) > i) for i in range(len(calls))]
    assert any(c["lengths"] is not None for c in calls)
    for c in calls:
        assert c["lengths"] is None or (len(c["lengths"]) == c["B"] and max(c["lengths"]) <= c["T"] and min(c["lengths"]) < c["T"])
    # content behind a chain's end never reaches it
    audio2, cond2 = audio.clone(), {k: v.clone() for k, v in cond.items()}
    for b, n in enumerate(lens):
        audio2[b, n:] = 1e4
        cond2["pretrain_aud_feat"][b, n:] = -1e4
    outs2 = tr.sample_arbitrary_len(audio2, pid, cond2, seed=7, row_keys=keys, lengths=lens)
    assert all(torch.equal(a, b) for a, b in zip(outs, outs2))
    # fix_very_first per chain: window 0 pinned to the chain's own first ground-truth window
    tr.opt.fix_very_first = True
    one.opt.fix_very_first = True
    motions = torch.randn(len(lens), N, cfg.net_dim_pose, generator=g)
    if min(lens) < L:                                        # (SHOW: the 5-frame chain has no overlap_len frames to pin)
        with pytest.raises(ValueError):
            tr.sample_arbitrary_len(audio, pid, cond, seed=7, row_keys=keys, lengths=lens, motions=motions)
    lens = [n if n >= L else L + 1 for n in lens]
    outs3 = tr.sample_arbitrary_len(audio, pid, cond, seed=7, row_keys=keys, lengths=lens, motions=motions)
    for b, n in enumerate(lens):
        want = one.sample_arbitrary_len(audio[b:b + 1, :n], pid[b:b + 1], {k: v[b:b + 1, :n] for k, v in cond.items()}, seed=7, row_keys=[keys[b]],
                                        motions=motions[b:b + 1, :n])[0]
        assert torch.equal(outs3[b], want), (b, n)
    tr.opt.fix_very_first = False
    tr.opt.same_overlap_noisy = True
    with pytest.raises(NotImplementedError):
        tr.sample_arbitrary_len(audio, pid, cond, seed=7, row_keys=keys, lengths=lens)
    tr.opt.same_overlap_noisy = False
    with pytest.raises(ValueError):
        tr.sample_arbitrary_len(audio, pid, cond, seed=7, row_keys=keys, lengths=lens[:-1])
    with pytest.raises(ValueError):
        tr.sample_arbitrary_len(audio, pid, cond, seed=7, row_keys=keys, lengths=[N + 1] + lens[1:])


@pytest.mark.parametrize("N,n_seg,max_rows", [(9000, 32, 64), (9000, 32, 5), (1000, 5, 64), (400, 8, 64), (300, 1, 64)])
def test_ragged_sharding_world1(N, n_seg, max_rows):
    from diffsheg_amd.trainer import split_segments, window_lengths
    cfg = get_config("show")
    audio, cond, pid = stream_inputs(cfg, N)
    segs = split_segments(N, n_seg, cfg.n_poses, cfg.overlap_len)
    one = stub_trainer(cfg)
    want = torch.cat([_alone(one, audio, cond, pid, s, i, 11) for i, s in enumerate(segs)], 0).unsqueeze(0)
    calls = []
    tr = stub_trainer(cfg, calls)
    got = tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=11, ragged=True, max_chains_per_batch=max_rows)
    assert got.shape == (1, N, cfg.net_dim_pose) and torch.equal(got, want)
    # sequential windows: the longest chain of every chunk, instead of the sum over the distinct lengths
    step = cfg.n_poses - cfg.overlap_len
    chunks = [segs[c0:c0 + max_rows] for c0 in range(0, len(segs), max_rows)]
    assert len(calls) == sum(max(len(window_lengths(len(s), cfg.n_poses, step)) for s in ch) for ch in chunks)
    n_ragged = len(calls)
    # ragged=False: exactly today's calls (no `lengths` anywhere) and today's stream
    del calls[:]
    off = tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=11, max_chains_per_batch=max_rows)
    assert torch.equal(off, want) and all(c["lengths"] is None for c in calls)
    by_len = {}
    for i, s in enumerate(segs):
        by_len.setdefault(len(s), []).append(i)
    exp = []
    for ids in by_len.values():
        for c0 in range(0, len(ids), max_rows):
            ch = ids[c0:c0 + max_rows]
            exp += [(len(ch), ln, ch) for ln in window_lengths(len(segs[ch[0]]), cfg.n_poses, step)]
    assert [(c["B"], c["T"], c["row_keys"]) for c in calls] == exp
    n_off = len(calls)
    assert torch.equal(off, tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=11, ragged=False, max_chains_per_batch=max_rows))
    if (N, n_seg, max_rows) == (9000, 32, 64):
        assert (n_off, n_ragged) == (11, 4)           # 19 x 312 + 12 x 234 + 1 x 264 frames: 4 + 3 + 4 windows against 4
    # seam repair runs behind the ragged chains, unchanged: frames outside the seam windows are the un-repaired ragged stream
    from diffsheg_amd.trainer import seam_windows, split_segments_for_repair
    rep = tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=11, ragged=True, seam_repair=True, max_chains_per_batch=max_rows)
    assert torch.equal(rep, tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=11, seam_repair=True, max_chains_per_batch=max_rows))
    segs_r = split_segments_for_repair(N, n_seg, cfg.n_poses, cfg.overlap_len)
    if len(segs_r) == len(segs):
        keep = torch.ones(N, dtype=torch.bool)
        for w in seam_windows(segs_r, cfg.n_poses):
            keep[w.start:w.stop] = False
        assert torch.equal(rep[:, keep], got[:, keep])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, N, n_seg, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = get_config("show")
        tr = stub_trainer(cfg)
        audio, cond, pid = stream_inputs(cfg, N)
        res = {}
        for name, kw in (("ragged", {"ragged": True}), ("ragged_chunked", {"ragged": True, "max_chains_per_batch": 2}),
                         ("ragged_repair", {"ragged": True, "seam_repair": True})):
            out = tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=11, **kw)
            assert (out is None) == (rank != 0)
            res[name] = None if out is None else out.numpy().copy()
        q.put((rank, res))
    finally:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.parametrize("N,n_seg", [(1000, 5), (9000, 32)])
def test_ragged_sharding_world2_equals_world1(N, n_seg):
    cfg = get_config("show")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, N, n_seg, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    tr = stub_trainer(cfg)
    audio, cond, pid = stream_inputs(cfg, N)
    one = tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=11, ragged=True)
    assert torch.equal(one, tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=11))
    two = {k: torch.from_numpy(v) for k, v in got[0].items()}
    assert torch.equal(two["ragged"], one) and torch.equal(two["ragged_chunked"], one)
    assert torch.equal(two["ragged_repair"], tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=11, ragged=True, seam_repair=True))


# ---- 3. the oracle property the kernels implement -------------------------------------------------------------------------------
def test_masked_padded_evaluation_equals_the_clips_alone():
    """SHOW weights, T_pad = 88, lengths 88 / 61 / 19 / 4.  With the three masks (attention K / V, HuBERT input, conv1 output) every row
    of ONE padded evaluation equals the clip evaluated alone at its length to fp32 round-off (gate: 2e-6 of the output range, the
    bound of tests/test_oracle_golden.py; measured 4.5e-7) — also with garbage in every padded frame.  Without the conv1-output mask
    the last valid frame is off by more than 1e-3 of the range: BatchNorm + GELU of a zero input is not zero."""
    from oracle import denoiser_ref as R
    cfg, sd = get_config("show"), synthetic_sd("show")
    T, lens = 88, [88, 61, 19, 4]
    B = len(lens)
    clips = clips_alone(cfg, lens)
    pid = person_ids(clips)
    t = torch.full((B,), 520, dtype=torch.long)
    c1, c2 = torch.full((B, 1, 1), 1.7), torch.full((B, 1, 1), 1.3)
    with torch.no_grad():
        ref = [R.unidiffuser(sd, cfg, c["x_T"], t[:1], c1[:1], c2[:1], c["audio_emb"], c["person_id"], c["pretrain_aud_feat"]) for c in clips]
    rng = max(float(r.max() - r.min()) for r in ref)

    def run(fill, **masks):
        with masked_oracle(lens, T, **masks), torch.no_grad():
            out = R.unidiffuser(sd, cfg, pad_batch(clips, "x_T", T, fill), t, c1, c2, pad_batch(clips, "audio_emb", T, fill), pid,
                                pad_batch(clips, "pretrain_aud_feat", T, fill))
        return ([float((out[i, :n] - ref[i][0]).abs().max()) / rng for i, n in enumerate(lens)],
                [float((out[i, n - 1] - ref[i][0, n - 1]).abs().max()) / rng for i, n in enumerate(lens)])
    for fill in (0.0, 7.0, 1.0e4):
        errs, _ = run(fill)
        print(f"[ragged oracle] pad fill {fill}: max err / range per row {['%.1e' % e for e in errs]}")
        assert max(errs) <= 2e-6, (fill, errs)
    errs, last = run(0.0, conv1=False)
    print(f"[ragged oracle] no conv1-output mask: rows {['%.1e' % e for e in errs]}, last valid frame {['%.1e' % e for e in last]}")
    assert all(e > 1e-3 for e in last[1:]) and errs[0] <= 2e-6
    errs, _ = run(0.0, attention=False, conv1=False, hubert_in=False)
    assert all(e > 1e-2 for e in errs[1:])


# ---- exports -----------------------------------------------------------------------------------------------------------------------
def test_ragged_exports_are_declared_and_bound():
    from diffsheg_amd import _lib
    from diffsheg_amd.model import UniDiffuser, normalize_lengths
    from diffsheg_amd.trainer import DDPMTrainer, sample_arbitrary_len_sharded
    header = open(os.path.join(ROOT, "include", "diffsheg_hip.h")).read()
    for name in ("dsh_set_condition_ragged", "dsh_op_linear_attention_ragged"):
        assert name in _lib.SYMBOLS, name
        assert f"int {name}(" in header, name
    assert "lengths" in inspect.signature(UniDiffuser.set_condition).parameters
    assert "lengths" in inspect.signature(DDPMTrainer.generate_batch).parameters
    assert "lengths" in inspect.signature(DDPMTrainer.sample_arbitrary_len).parameters
    assert inspect.signature(sample_arbitrary_len_sharded).parameters["ragged"].default is False
    assert normalize_lengths(None, 3, 8) is None and normalize_lengths(torch.full((3,), 8), 3, 8) is None
    assert normalize_lengths([8, 3, 1], 3, 8) == (8, 3, 1)
    for bad in ([8, 0, 1], [9, 3, 1], [8, 3]):
        with pytest.raises(ValueError):
            normalize_lengths(bad, 3, 8)
