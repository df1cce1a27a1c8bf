"""CPU tests (-m "not gpu") of two-sided in-betweening and of the seam repair of multi-chain streams: the two-sided fixtures
against the oracle, the seam geometry, the repair harness through gloo with a stub sampler (world 2 == world 1), and the new
exports."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from diffsheg_amd.config import get_config
from diffsheg_amd.synthetic import make_inputs
from util import golden, synthetic_sd

torch.set_num_threads(min(8, os.cpu_count() or 1))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the fixtures are what the (unchanged) oracle computes --------------------------------------------------------------
def twosided_inputs(cfg, f):
    """The fixture's inputs from its seeds: conditioning, and gt / mask with the first and the last L frames pinned (head drawn
    first, then tail, from one generator)."""
    B, L = int(f["batch"]), cfg.overlap_len
    assert L == int(f["overlap_len"])
    inp = make_inputs(cfg, B, seed=int(f["input_seed"]))
    g = torch.Generator().manual_seed(int(f["gt_seed"]))
    gt = torch.zeros(B, cfg.n_poses, cfg.net_dim_pose)
    gt[:, :L] = torch.randn(B, L, cfg.net_dim_pose, generator=g)
    gt[:, -L:] = torch.randn(B, L, cfg.net_dim_pose, generator=g)
    mask = torch.zeros_like(gt, dtype=torch.bool)
    mask[:, :L] = True
    mask[:, -L:] = True
    return B, inp, gt, mask


@pytest.mark.parametrize("ds,gate", [("show", 1e-6), ("beat", 2e-6)])
def test_oracle_reproduces_twosided_fixture(ds, gate):
    """The reference's out-painting loop on a mask pinned at both ends (addBlend, jump (3, 5)); gates of
    tests/test_oracle_golden.py for ddim25_harmonize_show_* (1e-6 of the output range) and ddim25_harmonize_beat_3_5 (2e-6)."""
    from oracle import denoiser_ref as D
    from oracle import sampler_ref as S
    cfg, sd = get_config(ds), synthetic_sd(ds)
    f = golden(f"ddim25_twosided_{ds}.npz")
    B, inp, gt, mask = twosided_inputs(cfg, f)
    L = cfg.overlap_len

    def eps_fn(x, t, c1, c2):
        with torch.no_grad():
            return D.unidiffuser(sd, cfg, x, torch.full((B,), t), c1, c2, inp["audio_emb"], inp["person_id"], inp["pretrain_aud_feat"])
    src = S.NoiseSource(seed=int(f["noise_seed"]))
    x = S.ddim_sample_loop(eps_fn, (B, cfg.n_poses, cfg.net_dim_pose), {"gt": gt, "outpainting_mask": mask}, src, overlap_len=L)
    assert src.i == int(f["draws"]) == 175
    scale = float(np.abs(f["final"]).max())
    err = float((x - torch.from_numpy(f["final"])).abs().max())
    print(f"[two-sided {ds}] oracle vs fixture: max err {err:.3e} = {err / scale:.3e} of the range {scale:.4g}")
    assert err <= gate * scale
    # the reference fades on the head side only: the pinned tail and head frame 0 (fade weight 0) are gt itself
    final = torch.from_numpy(f["final"])
    assert torch.allclose(final[:, -L:], gt[:, -L:], atol=1e-5) and torch.allclose(final[:, 0], gt[:, 0], atol=1e-5)


# ---- 2. seam geometry --------------------------------------------------------------------------------------------------------
def _fits(segs, n_poses, L, N):
    """Written from the definition: windows [p - n_poses // 2, + n_poses) inside the stream, pairwise disjoint."""
    wins = [(s.start - n_poses // 2, s.start - n_poses // 2 + n_poses) for s in segs[1:]]
    inside = all(a >= 0 and b <= N for a, b in wins)
    disjoint = all(wins[i][1] <= wins[i + 1][0] for i in range(len(wins) - 1))
    return inside and disjoint


GEOMETRY = [(9000, 32, 88, 10), (1000, 4, 88, 10), (9000, 256, 88, 10), (400, 8, 88, 10), (200, 2, 88, 10), (300, 3, 88, 10),
            (100, 3, 88, 10), (9000, 32, 34, 4), (9000, 400, 34, 4), (130, 6, 34, 4), (70, 2, 34, 4)]


@pytest.mark.parametrize("N,n_seg,n_poses,L", GEOMETRY)
def test_seam_geometry(N, n_seg, n_poses, L):
    from diffsheg_amd.trainer import seam_windows, split_segments, split_segments_for_repair
    base = split_segments(N, n_seg, n_poses, L)
    segs = split_segments_for_repair(N, n_seg, n_poses, L)
    assert segs[0].start == 0 and segs[-1].stop == N and all(a.stop == b.start for a, b in zip(segs[:-1], segs[1:]))
    wins = seam_windows(segs, n_poses)
    assert len(wins) == len(segs) - 1 and all(len(w) == n_poses for w in wins)
    assert _fits(segs, n_poses, L, N)
    for s, w in enumerate(wins):
        assert w.start == segs[s + 1].start - n_poses // 2
        # pinned frames: the first L of the window lie in the LEFT segment, the last L in the RIGHT one
        assert segs[s].start <= w.start and w.start + L <= segs[s].stop
        assert segs[s + 1].start <= w.stop - L and w.stop <= segs[s + 1].stop
    # the count is lowered only when it has to be, and only as far as it has to be
    if _fits(base, n_poses, L, N):
        assert segs == base
    else:
        assert any(len(s) < n_poses for s in base)
        want = next(k for k in range(len(base) - 1, 0, -1) if _fits(split_segments(N, k, n_poses, L), n_poses, L, N))
        assert len(segs) == want < len(base) and segs == split_segments(N, want, n_poses, L)
    # the default mode's split is not touched
    assert split_segments(N, n_seg, n_poses, L) == base


def test_geometry_cases_cover_clamped_and_unclamped_counts():
    from diffsheg_amd.trainer import split_segments, split_segments_for_repair
    assert len(split_segments_for_repair(9000, 32, 88, 10)) == 32 and len(split_segments_for_repair(9000, 32, 34, 4)) == 32
    assert min(len(s) for s in split_segments(9000, 256, 88, 10)) == 78 and min(len(s) for s in split_segments(400, 8, 88, 10)) == 78
    assert len(split_segments_for_repair(9000, 256, 88, 10)) < len(split_segments(9000, 256, 88, 10))
    assert len(split_segments_for_repair(400, 8, 88, 10)) < len(split_segments(400, 8, 88, 10))


# ---- stub sampler (the pattern of tests/test_distributed_cpu.py) -------------------------------------------------------------
class _StubTrainer:
    """DDPMTrainer with generate_batch replaced by a CPU function of (conditioning window, row key, seed, gt / mask): every frame of
    a row depends on the row's key, on the seed and on ALL of its pinned frames, so a wrong key, a wrong window of conditioning or a
    pinned frame taken from the wrong place changes the whole window.  Everything above generate_batch is the product code."""

    def __new__(cls, cfg, calls=None):
        from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace

        class Stub(DDPMTrainer):
            def __init__(self, opt):
                self.opt, self.device = opt, torch.device("cpu")

            def generate_batch(self, audio_emb, p_id, dim_pose, add_cond={}, inpaint_dict=None, seed=None, row_keys=None, **kw):
                B, T = audio_emb.shape[:2]
                if calls is not None:
                    calls.append({"B": B, "T": T, "y": inpaint_dict, "seed": seed, "row_keys": list(row_keys), "kw": dict(kw)})
                out = torch.empty(B, T, dim_pose)
                for b in range(B):
                    g = torch.Generator().manual_seed((int(seed) * 1000003 + int(row_keys[b])) & ((1 << 62) - 1))
                    out[b] = (torch.randn(T, dim_pose, generator=g) + audio_emb[b].mean(-1, keepdim=True)
                              + add_cond["pretrain_aud_feat"][b].mean(-1, keepdim=True) + p_id[b].argmax())
                m = (inpaint_dict or {}).get("outpainting_mask")
                if m is not None and bool(m.any()):
                    gt = inpaint_dict["gt"]
                    wt = torch.linspace(0.5, 1.5, T * dim_pose).view(1, T, dim_pose)          # position-dependent: swapped frames show
                    out = out + 0.01 * (gt * wt * m).sum((1, 2), keepdim=True)
                    out = torch.where(m, 0.5 * gt + 0.5 * out, out)
                    if kw.get("tail_blend"):
                        out = out + 0.125
                return out
        return Stub(sampler_namespace(cfg))


def _stream_inputs(cfg, N):
    g = torch.Generator().manual_seed(5)
    return (torch.randn(1, N, cfg.audio_dim, generator=g), {"pretrain_aud_feat": torch.randn(1, N, 16, generator=g)},
            torch.eye(cfg.style_dim)[1:2])


def test_sample_inbetween_builds_a_mask_pinned_at_both_ends():
    cfg = get_config("show")
    calls = []
    tr = _StubTrainer(cfg, calls)
    L, C, T = cfg.overlap_len, cfg.net_dim_pose, 60
    audio, cond, pid = _stream_inputs(cfg, T)
    g = torch.Generator().manual_seed(1)
    head, tail = torch.randn(1, L, C, generator=g), torch.randn(1, L, C, generator=g)
    out = tr.sample_inbetween(audio, pid, cond, head, tail, seed=3, row_keys=[7])
    assert out.shape == (1, T, C)
    y = calls[-1]["y"]
    want = torch.zeros(1, T, C, dtype=torch.bool)
    want[:, :L] = True
    want[:, -L:] = True
    assert torch.equal(y["outpainting_mask"], want) and y["outpainting_mask_any"] is True
    assert torch.equal(y["gt"][:, :L], head) and torch.equal(y["gt"][:, -L:], tail) and float(y["gt"][:, L:-L].abs().max()) == 0.0
    assert calls[-1]["kw"]["tail_blend"] is True and calls[-1]["seed"] == 3 and calls[-1]["row_keys"] == [7]
    tr.sample_inbetween(audio, pid, cond, head, tail, seed=3, row_keys=[7], tail_blend=False)
    assert calls[-1]["kw"]["tail_blend"] is False
    with pytest.raises(ValueError):
        tr.sample_inbetween(audio[:, :2 * L], pid, {k: v[:, :2 * L] for k, v in cond.items()}, head, tail, seed=3, row_keys=[7])
    with pytest.raises(ValueError):
        tr.sample_inbetween(audio, pid, cond, head[:, :-1], tail, seed=3, row_keys=[7])


def _expected_repair(tr, cfg, audio, cond, pid, N, n_seg, seed, tail_blend=True):
    """Seam repair written out seam by seam from the issue's definition, on top of the un-repaired stream."""
    from diffsheg_amd.trainer import SEAM_WINDOW, split_segments_for_repair, window_seed
    n_poses, L = cfg.n_poses, cfg.overlap_len
    segs = split_segments_for_repair(N, n_seg, n_poses, L)
    # the chains of the (possibly lowered) segment count, each sampled alone
    out = torch.cat([tr.sample_arbitrary_len(audio[:, s.start:s.stop], pid, {k: v[:, s.start:s.stop] for k, v in cond.items()},
                                             seed=seed, row_keys=[i]) for i, s in enumerate(segs)], 1)
    plain = out.clone()
    wins = []
    for s in range(len(segs) - 1):
        p = segs[s + 1].start
        a, b = p - n_poses // 2, p - n_poses // 2 + n_poses
        wins.append((a, b))
        out[:, a:b] = tr.sample_inbetween(audio[:, a:b], pid, {k: v[:, a:b] for k, v in cond.items()}, plain[:, a:a + L], plain[:, b - L:b],
                                          seed=window_seed(seed, SEAM_WINDOW), row_keys=[s], tail_blend=tail_blend)
    return plain, out, wins


@pytest.mark.parametrize("N,n_seg,max_rows", [(9000, 32, 64), (9000, 32, 5), (1000, 4, 64), (400, 8, 64), (300, 1, 64)])
def test_seam_repair_world1_equals_the_definition(N, n_seg, max_rows):
    from diffsheg_amd.trainer import split_segments
    cfg = get_config("show")
    calls = []
    tr = _StubTrainer(cfg, calls)
    audio, cond, pid = _stream_inputs(cfg, N)
    plain, want, wins = _expected_repair(_StubTrainer(cfg), cfg, audio, cond, pid, N, n_seg, 11)
    del calls[:]
    got = tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=11, seam_repair=True, max_chains_per_batch=max_rows)
    assert got.shape == (1, N, cfg.net_dim_pose) and torch.equal(got, want)
    # all seams of the rank are batched windows: rows = seams, chunked by max_chains_per_batch
    seam_calls = [c for c in calls if "tail_blend" in c["kw"]]
    assert [c["B"] for c in seam_calls] == [min(max_rows, len(wins) - i) for i in range(0, len(wins), max_rows)]
    assert sum((c["row_keys"] for c in seam_calls), []) == list(range(len(wins)))
    if wins:
        assert not torch.equal(got, plain)
    # default mode: what the parent returns (every chain of split_segments sampled alone, concatenated)
    off = tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=11)
    segs0 = split_segments(N, n_seg, cfg.n_poses, cfg.overlap_len)
    parent = torch.cat([tr.sample_arbitrary_len(audio[:, s.start:s.stop], pid, {k: v[:, s.start:s.stop] for k, v in cond.items()},
                                                seed=11, row_keys=[i]) for i, s in enumerate(segs0)], 1)
    assert torch.equal(off, parent)
    assert torch.equal(off, tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=11, seam_repair=False))
    if len(segs0) == len(wins) + 1:            # same chains in both modes: frames outside the seam windows are untouched
        keep = torch.ones(N, dtype=torch.bool)
        for a, b in wins:
            keep[a:b] = False
        assert torch.equal(got[:, keep], off[:, keep])
    # seam_tail_blend reaches the window call
    nb = tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=11, seam_repair=True, seam_tail_blend=False)
    assert torch.equal(nb, _expected_repair(_StubTrainer(cfg), cfg, audio, cond, pid, N, n_seg, 11, tail_blend=False)[1])


def test_seam_repair_refuses_configurations_it_cannot_serve():
    cfg = get_config("show")
    audio, cond, pid = _stream_inputs(cfg, 400)
    tr = _StubTrainer(cfg)
    tr.opt.ddim = False
    with pytest.raises(ValueError):
        tr.sample_arbitrary_len_sharded(audio, pid, cond, 2, seed=1, seam_repair=True)
    tr = _StubTrainer(cfg)
    tr.opt.overlap_len = 0
    with pytest.raises(ValueError):
        tr.sample_arbitrary_len_sharded(audio, pid, cond, 2, seed=1, seam_repair=True)


# ---- 3. through gloo: world 2 == world 1 -------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sharded_worker(rank, world, port, N, n_seg, rank0_only, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = get_config("show")
        tr = _StubTrainer(cfg)
        audio, cond, pid = _stream_inputs(cfg, N)
        if rank0_only and rank != 0:
            audio, cond = None, None
        res = {}
        for name, kw in (("off", {}), ("on", {"seam_repair": True}), ("on_chunked", {"seam_repair": True, "max_chains_per_batch": 2})):
            out = tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=11, inputs_on_rank0_only=rank0_only, **kw)
            assert (out is None) == (rank != 0)
            res[name] = None if out is None else out.numpy().copy()      # by value (see tests/test_distributed_cpu.py)
        q.put((rank, res))
    finally:
        dist.barrier()
        dist.destroy_process_group()


# world 2: (1000, 5) = segments 0-2 | 3-4: seams 0, 1 on rank 0, seam 3 on rank 1, seam 2 on the rank boundary;
# (1000, 2) = the only seam is the rank boundary; (400, 8) = count lowered to 3; (300, 1) = one chain, no seam anywhere
@pytest.mark.parametrize("N,n_seg,rank0_only", [(1000, 5, False), (1000, 2, True), (400, 8, False), (300, 1, False)])
def test_seam_repair_world2_equals_world1(N, n_seg, rank0_only):
    from diffsheg_amd.trainer import shard_range, split_segments_for_repair
    cfg = get_config("show")
    segs = split_segments_for_repair(N, n_seg, cfg.n_poses, cfg.overlap_len)
    owner = {i: r for r in range(2) for i in shard_range(len(segs), r, 2)}
    on_boundary = [s for s in range(len(segs) - 1) if owner[s] != owner[s + 1]]
    assert len(on_boundary) == (1 if len(segs) > 1 else 0)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, N, n_seg, rank0_only, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    tr = _StubTrainer(cfg)
    audio, cond, pid = _stream_inputs(cfg, N)
    one_off = tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=11)
    one_on = tr.sample_arbitrary_len_sharded(audio, pid, cond, n_seg, seed=11, seam_repair=True)
    plain, want, wins = _expected_repair(tr, cfg, audio, cond, pid, N, n_seg, 11)
    two = {k: torch.from_numpy(v) for k, v in got[0].items()}
    assert torch.equal(two["off"], one_off)
    assert torch.equal(one_on, want)
    assert torch.equal(two["on"], one_on) and torch.equal(two["on_chunked"], one_on)
    if wins:
        assert not torch.equal(one_on, plain)


# ---- 4. exports ----------------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_and_bound():
    from diffsheg_amd import _lib
    header = open(os.path.join(ROOT, "include", "diffsheg_hip.h")).read()
    for name in ("dsh_sample_set_tail_blend", "dsh_op_ddim_step"):
        assert name in _lib.SYMBOLS, name
        assert f"int {name}(" in header, name
    import inspect
    from diffsheg_amd.diffusion import GaussianDiffusion
    assert inspect.signature(GaussianDiffusion._run).parameters["tail_blend"].default is False
