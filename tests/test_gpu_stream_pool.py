"""Live sessions on a real MI355X (diffsheg_amd.streaming.StreamPool): the per-row Philox seeds at op and loop level, the two hand-off
kernels against their torch expressions, a lone session against the offline chain bit for bit, sessions at different windows in one
call against each chain alone, and that nothing moved for callers that set no row seeds.  Gates for "a chain inside a batch against the
chain alone" are the project's own (tests/test_gpu_ragged.py): fp32 1e-5 of range, bf16 1.2e-2."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsheg_amd import _lib  # noqa: E402
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.glue import PoseStats  # noqa: E402
from diffsheg_amd.model import UniDiffuser  # noqa: E402
from diffsheg_amd.streaming import StreamPool, chain_handoff, chain_save_tail  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace, window_seed  # noqa: E402
from util import assert_split_ran, gpu_model, rel_err, synthetic_sd  # noqa: E402

DEV = "cuda:0"
LOOP_FP32, LOOP_BF16 = 1e-5, 1.2e-2


def _p(t):
    return C.c_void_p(t.data_ptr())


def _u64(vals):
    return (C.c_uint64 * len(vals))(*[int(v) & (2 ** 64 - 1) for v in vals])


def _dev_u64(vals):
    """64-bit keys as a device array (int64 storage, the same bits)."""
    return torch.tensor([v - 2 ** 64 if v >= 2 ** 63 else v for v in vals], dtype=torch.int64).to(DEV)


# ---- 1. Philox, op level ------------------------------------------------------------------------------------------------------------
def _rows(keys, n_row, seed, offset, lens=None, draw=0, channels=0, row_seeds=None):
    rows = len(keys)
    out = torch.full((rows, n_row), float("nan"), device=DEV)
    L = _lib.lib()
    larr = (C.c_int32 * rows)(*lens) if lens is not None else None
    sd = _dev_u64(row_seeds) if row_seeds is not None else None
    if row_seeds is None and lens is None:
        _lib.check(L.dsh_op_philox_randn_rows(None, _p(out), rows, n_row, seed, offset, _u64(keys)), "dsh_op_philox_randn_rows")
    elif row_seeds is None:
        _lib.check(L.dsh_op_philox_randn_rows_ragged(None, _p(out), rows, n_row, seed, offset, _u64(keys), larr, draw, channels),
                   "dsh_op_philox_randn_rows_ragged")
    elif lens is None:
        _lib.check(L.dsh_op_philox_randn_rows_seeded(None, _p(out), rows, n_row, seed, offset, _u64(keys), _p(sd)),
                   "dsh_op_philox_randn_rows_seeded")
    else:
        _lib.check(L.dsh_op_philox_randn_rows_ragged_seeded(None, _p(out), rows, n_row, seed, offset, _u64(keys), larr, draw, channels, _p(sd)),
                   "dsh_op_philox_randn_rows_ragged_seeded")
    torch.cuda.synchronize()
    return out.cpu()


def test_philox_row_seeds_op_level():
    rows, n_row, seed, off = 3, 8, 0x1234ABCD5678, 5
    keys = [11, 2 ** 63 + 5, 11]                       # rows 0 and 2 share a key
    seeds = [window_seed(7, 3), 2 ** 64 - 3, window_seed(7, 4)]
    plain = _rows(keys, n_row, seed, off)
    assert torch.isfinite(plain).all()
    # every row seed = the call's seed: the unseeded launch, exactly; and a NULL seed array is that launch itself
    assert torch.equal(_rows(keys, n_row, 999, off, row_seeds=[seed] * rows), plain)
    out = torch.empty(rows, n_row, device=DEV)
    _lib.check(_lib.lib().dsh_op_philox_randn_rows_seeded(None, _p(out), rows, n_row, seed, off, _u64(keys), None))
    assert torch.equal(out.cpu(), plain)
    # three different seeds: row b is the one-row call with (row_seeds[b], row_keys[b])
    z = _rows(keys, n_row, 999, off, row_seeds=seeds)
    for b in range(rows):
        assert torch.equal(z[b], _rows([keys[b]], n_row, seeds[b], off)[0]), b
    assert not torch.equal(z[0], z[2])                 # equal keys, different seeds
    assert not torch.equal(z[0], plain[0])
    # the ragged form: rows of 2, 1, 2 frames of 4 channels, third draw
    lens, ch, draw = [2, 1, 2], 4, 3
    rag = _rows(keys, n_row, seed, 0, lens, draw, ch)
    assert torch.equal(_rows(keys, n_row, 999, 0, lens, draw, ch, row_seeds=[seed] * rows), rag)
    zr = _rows(keys, n_row, 999, 0, lens, draw, ch, row_seeds=seeds)
    for b in range(rows):
        solo = _rows([keys[b]], n_row, seeds[b], 0, [lens[b]], draw, ch)
        assert torch.equal(zr[b, :lens[b] * ch], solo[0, :lens[b] * ch]), b
        alone = _rows([keys[b]], lens[b] * ch, seeds[b], draw * (lens[b] * ch // 4))       # the clip alone at its own length
        assert torch.equal(zr[b, :lens[b] * ch], alone[0]), b
    assert not torch.equal(zr[0, :8], zr[2, :8])


# ---- 2. hand-off kernels ------------------------------------------------------------------------------------------------------------
def _tails(S, L, Cc, seed=0):
    return torch.randn(S, L, Cc, generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.mark.parametrize("T,L", [(7, 3), (7, 6)])
def test_chain_handoff_and_save_tail_against_torch(T, L):
    S, Cc, slots = 5, 5, [4, 0, 2]
    R = len(slots)
    tails = _tails(S, L, Cc, 1)
    gt, mask = chain_handoff(tails, slots, T)
    ref_gt = torch.zeros(R, T, Cc, device=DEV)
    ref_gt[:, :L] = tails[slots]
    ref_mask = torch.zeros(R, T, Cc, dtype=torch.uint8, device=DEV)
    ref_mask[:, :L] = 1
    assert gt.dtype == torch.float32 and mask.dtype == torch.uint8
    assert torch.equal(gt, ref_gt) and torch.equal(mask, ref_mask)
    # save: full rows, then per-row lengths
    x = torch.randn(R, T, Cc, generator=torch.Generator().manual_seed(2)).to(DEV)
    for lens in (None, [7, max(4, L), max(5, L)]):
        table = _tails(S, L, Cc, 3)
        ref = table.clone()
        for r, s in enumerate(slots):
            n = T if lens is None else lens[r]
            ref[s] = x[r, n - L:n]
        chain_save_tail(x, slots, table, lens)
        assert torch.equal(table, ref), lens
    # R = 0: nothing is launched, the table stays
    table = _tails(S, L, Cc, 4)
    before = table.clone()
    chain_save_tail(torch.empty(0, T, Cc, device=DEV), [], table)
    g0, m0 = chain_handoff(table, [], T)
    torch.cuda.synchronize()
    assert torch.equal(table, before) and tuple(g0.shape) == (0, T, Cc) and tuple(m0.shape) == (0, T, Cc)


def test_chain_handoff_refusals_launch_nothing():
    S, T, L, Cc = 5, 7, 3, 5
    lib = _lib.lib()
    tails = _tails(S, L, Cc, 5)
    before = tails.clone()
    x = torch.ones(3, T, Cc, device=DEV)
    gt = torch.full((3, T, Cc), 7.0, device=DEV)
    mask = torch.full((3, T, Cc), 9, dtype=torch.uint8, device=DEV)
    i32 = lambda v: (C.c_int32 * len(v))(*v)              # noqa: E731
    dev = lambda v: torch.tensor(v, dtype=torch.int32).to(DEV)      # noqa: E731

    def handoff(slots, T_=T, L_=L):
        d = dev(slots)
        return lib.dsh_op_chain_handoff(None, _p(tails), S, i32(slots), _p(d), len(slots), T_, L_, Cc, _p(gt), _p(mask))

    def save(slots, T_=T, L_=L, lens=None):
        d = dev(slots)
        ld = dev(lens) if lens is not None else None
        return lib.dsh_op_chain_save_tail(None, _p(x), i32(lens) if lens is not None else None, _p(ld) if ld is not None else None,
                                          i32(slots), _p(d), len(slots), T_, L_, Cc, _p(tails), S)
    ok = [4, 0, 2]
    cases = [(lambda: handoff(ok, L_=0), b"overlap_len"), (lambda: handoff(ok, T_=3, L_=3), b"overlap_len"), (lambda: handoff(ok, T_=2, L_=3), b"overlap_len"),
             (lambda: handoff([4, 5, 2]), b"slot"), (lambda: handoff([4, -1, 2]), b"slot"),
             (lambda: save(ok, L_=0), b"overlap_len"), (lambda: save(ok, T_=3, L_=3), b"overlap_len"), (lambda: save([4, 5, 2]), b"slot"),
             (lambda: save([-1, 0, 2]), b"slot"), (lambda: save([4, 0, 4]), b"twice"), (lambda: save(ok, lens=[7, 2, 5]), b"length"),
             (lambda: save(ok, lens=[7, 8, 5]), b"length")]
    for i, (call, word) in enumerate(cases):
        rc = call()
        assert rc == -1 and word in lib.dsh_last_error(), (i, rc, word, lib.dsh_last_error())
    torch.cuda.synchronize()
    assert torch.equal(tails, before) and bool((gt == 7.0).all()) and bool((mask == 9).all())
    assert handoff(ok) == 0 and save(ok) == 0             # ... and the same arguments without the fault run
    torch.cuda.synchronize()
    assert bool((mask[:, :L] == 1).all()) and bool((tails[ok] == 1.0).all())
    with pytest.raises(_lib.DshError):
        chain_handoff(tails, [0, S], T)
    with pytest.raises(_lib.DshError):
        chain_save_tail(x, [1, 1, 2], tails)


# ---- helpers of the pool tests --------------------------------------------------------------------------------------------------------
def _features(cfg, N, seed, speaker):
    inp = make_inputs(cfg, 1, frames=N, seed=seed)
    pid = torch.zeros(cfg.style_dim)
    pid[speaker % cfg.style_dim] = 1.0
    return inp["audio_emb"][0].to(DEV), inp["pretrain_aud_feat"][0].to(DEV), pid.to(DEV)


def _offline(tr, a, h, pid, seed, key, cond_scale=None, **kw):
    return tr.sample_arbitrary_len(a[None], pid[None], {"pretrain_aud_feat": h[None]}, seed=seed, row_keys=[key], cond_scale=cond_scale, **kw)[0]


def _count_calls(tr, monkeypatch, launch_counts=False):
    """(clips, frames) of every sampler call; launch_counts: and the library's launch counters of that call as a third entry."""
    calls = []
    orig = tr.generate_batch

    def counted(*a, **k):
        if not launch_counts:
            calls.append((int(a[0].shape[0]), int(a[0].shape[1])))
            return orig(*a, **k)
        _lib.launch_counts(reset=True)
        out = orig(*a, **k)
        torch.cuda.synchronize()
        calls.append((int(a[0].shape[0]), int(a[0].shape[1]), _lib.launch_counts()))
        return out
    monkeypatch.setattr(tr, "generate_batch", counted)
    return calls


class _Sessions:
    """The bookkeeping of the pool tests: sessions by name over their features (audio, HuBERT, speaker), the frames fed and the frames
    emitted so far, and the sampler calls of every step()."""

    def __init__(self, tr, pool, feat, monkeypatch, launch_counts=False):
        self.pool, self.feat = pool, feat
        self.sid, self.fed, self.got = {}, {n: 0 for n in feat}, {n: [] for n in feat}
        self.calls = _count_calls(tr, monkeypatch, launch_counts)

    def open(self, n, **kw):
        self.sid[n] = self.pool.open(self.feat[n][2], **kw)

    def feed(self, n, k):
        a, h, _ = self.feat[n]
        self.pool.feed(self.sid[n], a[self.fed[n]:self.fed[n] + k], {"pretrain_aud_feat": h[self.fed[n]:self.fed[n] + k]})
        self.fed[n] += k

    def step(self, expect_calls):
        del self.calls[:]
        out = self.pool.step()
        assert sorted(c[:2] for c in self.calls) == sorted(expect_calls), ([c[:2] for c in self.calls], expect_calls)
        for n, s_ in self.sid.items():
            if s_ in out:
                self.got[n].append(out[s_])
        return out


# ---- 3. a lone session is the offline chain, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("N", [34 + 30 + 17, 34 + 30, 20])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_lone_session_is_the_offline_chain_bit_for_bit(precision, N):
    """BEAT, jump_n_sample = 2: two full windows and a tail / no fractional window (close flushes the held-back frames) / one short
    window.  Fed in chunks of 13 frames with a step() behind every feed."""
    cfg = get_config("beat")
    tr = DDPMTrainer(sampler_namespace(cfg, jump_n_sample=2), gpu_model("beat", precision))
    a, h, pid = _features(cfg, N, 60 + N, 3)
    seed, key = 2024, 77
    want = _offline(tr, a, h, pid, seed, key)
    assert tuple(want.shape) == (N, cfg.net_dim_pose)
    pool = StreamPool(tr, 2, seed)
    sid = pool.open(pid, key=key)
    got, n_emits = [], 0
    for c0 in range(0, N, 13):
        pool.feed(sid, a[c0:c0 + 13].cpu() if c0 == 13 else a[c0:c0 + 13], {"pretrain_aud_feat": h[c0:c0 + 13]})      # (host or device)
        out = pool.step()
        assert set(out) <= {sid}
        if out:
            assert tuple(out[sid].shape) == (cfg.n_poses - cfg.overlap_len, cfg.net_dim_pose)
            got.append(out[sid])
            n_emits += 1
        assert pool._sessions[sid].audio.shape[0] < cfg.n_poses        # consumed audio is dropped
    assert pool.step() == {}
    got.append(pool.close(sid))
    assert n_emits == {81: 2, 64: 2, 20: 0}[N] and len(pool) == 0
    full = torch.cat(got, 0)
    assert tuple(full.shape) == tuple(want.shape) and torch.isfinite(full).all()
    assert torch.equal(full, want), float((full - want).abs().max())
    if precision == "fp32" and N == 81:
        # pose_rep="euler" is the existing conversion on the emitted frames
        tr.set_pose_stats(PoseStats(*(torch.randn(cfg.dim_pose, generator=torch.Generator().manual_seed(i)) * s + o
                                      for i, (s, o) in enumerate(((0.1, 0.0), (0.05, 0.6), (10.0, 0.0), (3.0, 20.0))))))
        pool = StreamPool(tr, 1, seed)
        sid = pool.open(pid, key=key)
        pool.feed(sid, a, {"pretrain_aud_feat": h})
        eul = []
        while True:
            out = pool.step(pose_rep="euler")
            if not out:
                break
            eul.append(out[sid])
        eul.append(pool.close(sid, pose_rep="euler"))
        assert len(eul) == 3 and torch.equal(torch.cat(eul, 0), tr._to_euler(want))


# ---- 4. sessions at different windows in one call -------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sessions_at_different_windows_share_one_call(precision, monkeypatch):
    """SHOW, jump_n_sample = 2.  Three sessions (speakers 0 / 1 / 2, their own keys and guidance scales) opened one step() apart: the
    fourth step() holds windows 3, 2 and 1 in ONE chained call.  A ends in a tail while B and C go on; B ends exactly on a window
    (flush), C in another tail, closed together."""
    cfg = get_config("show")
    tr = DDPMTrainer(sampler_namespace(cfg, jump_n_sample=2), gpu_model("show", precision))
    size, L = cfg.n_poses, cfg.overlap_len
    st = size - L
    total = {"A": size + 3 * st + 30, "B": size + 3 * st, "C": size + 2 * st + 25}
    spec = {"A": (0, 901, 1.25), "B": (1, 17, 1.0), "C": (2, 2 ** 40 + 3, 2.0)}      # speaker, key, cond_scale
    feat = {n: _features(cfg, total[n], 80 + i, spec[n][0]) for i, n in enumerate("ABC")}
    seed = 555
    pool = StreamPool(tr, 3, seed)
    ss = _Sessions(tr, pool, feat, monkeypatch)
    calls, sid, fed, got, feed, step = ss.calls, ss.sid, ss.fed, ss.got, ss.feed, ss.step
    for tick, name in enumerate("ABC"):
        ss.open(name, key=spec[name][1], cond_scale=spec[name][2])
        feed(name, size)
        for other in "ABC"[:tick]:
            feed(other, st)
        out = step([(1, size)] + ([(tick, size)] if tick else []))           # one plain call, one chained call
        assert len(out) == tick + 1
    with pytest.raises(RuntimeError, match="full"):
        pool.open(feat["A"][2])
    for n in "ABC":
        feed(n, st)
    assert [pool._sessions[sid[n]].win.windows for n in "ABC"] == [3, 2, 1]
    assert len(step([(3, size)])) == 3                                           # windows 3, 2 and 1: ONE sampler call
    feed("A", 30)
    del calls[:]
    got["A"].append(pool.close(sid["A"]))                                        # A's tail window runs in its close ...
    assert calls == [(1, L + 30)]
    feed("B", st)
    feed("C", st)
    assert len(step([(2, size)])) == 2                                           # ... while B and C go on
    feed("C", 25)
    del calls[:]
    rest = pool.close_many([sid["B"], sid["C"]])
    assert calls == [(1, L + 25)] and len(pool) == 0                             # B: held-back frames, no sampling
    got["B"].append(rest[sid["B"]])
    got["C"].append(rest[sid["C"]])
    monkeypatch.undo()
    tol = LOOP_FP32 if precision == "fp32" else LOOP_BF16
    worst = 0.0
    for n in "ABC":
        a, h, pid = feat[n]
        stream = torch.cat(got[n], 0)
        assert fed[n] == total[n] and tuple(stream.shape) == (total[n], cfg.net_dim_pose) and torch.isfinite(stream).all()
        solo = _offline(tr, a, h, pid, seed, spec[n][1], spec[n][2])
        e = rel_err(stream, solo)
        print(f"[stream pool {precision}] session {n} ({total[n]} frames) vs its chain alone offline: rel err {e:.3e} (gate {tol:.1e})")
        worst = max(worst, e)
    # noise that ignored the row seeds could not pass: the same chain with another seed is a different stream
    a, h, pid = feat["A"]
    other = rel_err(torch.cat(got["A"], 0), _offline(tr, a, h, pid, seed + 1, spec["A"][1], spec["A"][2]))
    print(f"[stream pool {precision}] worst rel err {worst:.3e} (gate {tol:.1e}); against the chain of another seed {other:.3e}")
    assert worst < tol
    assert other > tol


def _seven_sessions(tr, feats, seed, late, monkeypatch):
    """Six sessions opened together and (late) a seventh one step() behind them, SHOW windows of 88 frames: the calls are (6, 88) plain; (1, 88)
    plain for the late session beside (6, 88) chained; (6 or 7, 88) chained with the sessions at different windows; close_many flushes the
    held-back frames.  Returns (the stream of every session, the late session's first emission, per sampler call (clips, frames, launch counts))."""
    cfg = tr.encoder.cfg
    size, st = cfg.n_poses, cfg.n_poses - cfg.overlap_len
    n = 7 if late else 6
    pool = StreamPool(tr, n, seed)
    ss = _Sessions(tr, pool, dict(enumerate(feats[:n])), monkeypatch, launch_counts=True)
    log = []
    for i in range(6):
        ss.open(i, key=1000 + i)
        ss.feed(i, size)
    ss.step([(6, size)])
    log += ss.calls
    if late:
        ss.open(6, key=1006)
        ss.feed(6, size)
    for i in range(6):
        ss.feed(i, st)
    ss.step([(6, size)] + ([(1, size)] if late else []))
    log += ss.calls
    first_of_late = ss.got[6][0].clone() if late else None
    for i in range(n):
        ss.feed(i, st)
    assert [pool._sessions[ss.sid[i]].win.windows for i in range(n)] == [2] * 6 + [1] * (n - 6)      # windows done so far
    ss.step([(n, size)])                                                         # the third and the second window: ONE sampler call
    log += ss.calls
    rest = pool.close_many([ss.sid[i] for i in range(n)])
    monkeypatch.undo()
    streams = [torch.cat(ss.got[i] + [rest[ss.sid[i]]], 0) for i in range(n)]
    for i, x in enumerate(streams):
        assert tuple(x.shape) == (ss.fed[i], cfg.net_dim_pose) and torch.isfinite(x).all()
    return streams, first_of_late, log


def test_sessions_share_one_call_on_the_split_loop(monkeypatch):
    """precision "bf16x3", SHOW, jump_n_sample = 2, enough sessions that a shared call is above the 512-row limit of the split-bf16 loop
    (6 x 88 = 528 rows).  ONE context goes above the limit (six sessions), below it (the late seventh session's first window: 88 rows, beside
    the six again), and above it again (all seven, at windows 3 and 2).
      * every call above the limit is on the split loop, the one below on the fp32 kernels - and its frames are the fp32 context's frames for
        the same session bit for bit;
      * the six early streams inside the pool of seven against the same sessions in a pool of six (both above the limit: the same
        arithmetic at another batch size) under the project's 1e-5 of the range;
      * every stream against the fp32 context's stream of the same choreography under 1e-3 of the range;
      * the distance to the chain sampled alone offline (which runs the fp32 kernels: it crosses the change of arithmetic) is printed.
    Eager evaluations (DSH_NO_GRAPH): the launch counters are host-side and see every launch of every call."""
    monkeypatch.setenv("DSH_NO_GRAPH", "1")
    cfg = get_config("show")
    size, st = cfg.n_poses, cfg.n_poses - cfg.overlap_len
    feats = [_features(cfg, size + 2 * st, 200 + i, i) for i in range(7)]
    seed = 777
    tr3 = DDPMTrainer(sampler_namespace(cfg, jump_n_sample=2), gpu_model("show", "bf16x3"))
    tr32 = DDPMTrainer(sampler_namespace(cfg, jump_n_sample=2), gpu_model("show", "fp32"))
    s7, late3, log = _seven_sessions(tr3, feats, seed, True, monkeypatch)
    monkeypatch.setenv("DSH_NO_GRAPH", "1")                                      # (_seven_sessions undoes its patches)
    assert [c[:2] for c in log if c[0] * c[1] <= 512] == [(1, size)]
    for nb, T, counts in log:
        if nb * T > 512:
            assert_split_ran(counts, (nb, T))
        else:
            assert counts["gemm_f32_split"] == 0, counts
    order = [c[0] * c[1] > 512 for c in log]
    assert order[0] and not all(order[1:3]) and order[-1], order                 # above, (below beside above), above
    s6, _, _ = _seven_sessions(tr3, feats, seed, False, monkeypatch)
    monkeypatch.setenv("DSH_NO_GRAPH", "1")
    f7, late32, log32 = _seven_sessions(tr32, feats, seed, True, monkeypatch)
    assert all(c[2]["gemm_f32_split"] == 0 for c in log32)
    assert torch.equal(late3, late32), "below the limit a bf16x3 context must launch the fp32 kernels"
    w6 = max(rel_err(s7[i], s6[i]) for i in range(6))
    w32 = max(rel_err(s7[i], f7[i]) for i in range(7))
    a, h, pid = feats[0]
    alone = rel_err(s7[0], tr3.sample_arbitrary_len(a[None], pid[None], {"pretrain_aud_feat": h[None]}, seed=seed, row_keys=[1000])[0])
    print(f"[measure] stream pool bf16x3: six sessions in a pool of 7 vs a pool of 6: {w6:.3e} (gate {LOOP_FP32:.1e}); vs the fp32 context: {w32:.3e} (gate 1.0e-03); "
          f"session 0 vs its chain alone offline (fp32 kernels, no gate): {alone:.3e}")
    assert w6 < LOOP_FP32
    assert w32 < 1e-3
    assert not torch.equal(s7[0], f7[0])


def test_tails_of_different_lengths_close_together():
    """close_many with tails of different lengths: one chained call with lengths=, every stream vs its chain alone (BEAT fp32)."""
    cfg = get_config("beat")
    tr = DDPMTrainer(sampler_namespace(cfg, jump_n_sample=2), gpu_model("beat", "fp32"))
    size, L = cfg.n_poses, cfg.overlap_len
    totals = [size + 9, size + 21, 12]                    # tails of L + 9 and L + 21 frames, and a short plain window
    feats = [_features(cfg, n, 130 + i, i) for i, n in enumerate(totals)]
    pool = StreamPool(tr, 3, 9)
    sids = [pool.open(f[2], key=300 + i) for i, f in enumerate(feats)]
    for s, (a, h, _) in zip(sids, feats):
        pool.feed(s, a, {"pretrain_aud_feat": h})
    rest = pool.close_many(sids)                          # takes the due first windows, then the two tails together and the short one
    worst = 0.0
    for i, (s, (a, h, pid)) in enumerate(zip(sids, feats)):
        assert tuple(rest[s].shape) == (totals[i], cfg.net_dim_pose)
        worst = max(worst, rel_err(rest[s], _offline(tr, a, h, pid, 9, 300 + i)))
    print(f"[stream pool close_many] worst rel err vs the chains alone {worst:.3e} (gate {LOOP_FP32:.1e})")
    assert worst < LOOP_FP32


# ---- 5. nothing else moved -----------------------------------------------------------------------------------------------------------
def _raw_sample(model, opts, shape, gt=None, mask=None):
    """dsh_sample straight through the C ABI on the condition and the sticky keys / seeds the context holds."""
    x = torch.empty(*shape, device=DEV)
    masked = int(gt is not None)
    _lib.check(_lib.lib().dsh_sample(model._h, C.byref(opts), _p(x), 0, _p(gt) if masked else None, _p(mask) if masked else None, masked, None, 0, None),
               "dsh_sample")
    torch.cuda.synchronize()
    return x


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_without_row_seeds_nothing_moved(precision):
    """A context that has never seen row seeds, the same context with seeds set (sticky across dsh_sample calls), and after
    dsh_sample_set_row_seeds(..., 0): a ddim25 loop with row keys and a chained window, bit for bit.  All row seeds = the call's seed is
    the unseeded loop exactly — every draw of the loop (x_T, the steps, the RePaint blend's gt noise, the undo steps, the eta draws; both
    encoder chains of the pipelined loop) honours the row's seed."""
    cfg = get_config("beat")
    model = UniDiffuser(cfg, synthetic_sd("beat"), device=DEV, precision=precision)         # a fresh context
    tr = DDPMTrainer(sampler_namespace(cfg, jump_n_sample=2), model)
    lib = _lib.lib()
    B, T, Cc, L = 3, cfg.n_poses, cfg.net_dim_pose, cfg.overlap_len
    inp = make_inputs(cfg, B, frames=T, seed=9)
    a, p, cnd = inp["audio_emb"].to(DEV), inp["person_id"].to(DEV), {"pretrain_aud_feat": inp["pretrain_aud_feat"].to(DEV)}
    keys, seed = [5, 6, 2 ** 50], 4242
    tails = _tails(B, L, Cc, 8)
    gt, mask = chain_handoff(tails, [0, 1, 2], T)
    y = {"gt": gt, "outpainting_mask": mask, "outpainting_mask_any": True}
    plain0 = tr.generate_batch(a, p, Cc, cnd, {}, seed=seed, row_keys=keys)
    chain0 = tr.generate_batch(a, p, Cc, cnd, dict(y), seed=seed, row_keys=keys)
    eta0 = tr.generate_batch(a, p, Cc, cnd, dict(y), seed=seed, row_keys=keys, eta=0.5)
    assert torch.isfinite(plain0).all() and torch.isfinite(chain0).all() and not torch.equal(chain0, eta0)
    # all seeds = the seed: the same loops, whatever opts.seed says
    assert torch.equal(tr.generate_batch(a, p, Cc, cnd, {}, seed=1, row_keys=keys, row_seeds=[seed] * B), plain0)
    assert torch.equal(tr.generate_batch(a, p, Cc, cnd, dict(y), seed=1, row_keys=keys, row_seeds=[seed] * B), chain0)
    assert torch.equal(tr.generate_batch(a, p, Cc, cnd, dict(y), seed=1, row_keys=keys, row_seeds=[seed] * B, eta=0.5), eta0)
    # different seeds: row b is the row sampled with (row_seeds[b], keys[b]) — here against the batch sampled with that seed for all
    seeds = [seed, seed + 1, window_seed(seed, 2)]
    same = {b: tr.generate_batch(a, p, Cc, cnd, dict(y), seed=seeds[b], row_keys=keys) for b in (1, 2)}
    mixed = tr.generate_batch(a, p, Cc, cnd, dict(y), seed=1, row_keys=keys, row_seeds=seeds)
    assert torch.equal(mixed[0], chain0[0]) and not torch.equal(mixed[1], chain0[1]) and not torch.equal(mixed[2], chain0[2])
    for b in (1, 2):
        assert torch.equal(mixed[b], same[b][b]), (b, rel_err(mixed[b], same[b][b]))
    # the loops above left nothing in the context (each carried its keys and seeds in its own dsh_run_spec) ...
    opts = tr.diffusion_ddim_val._opts(0, False, 1, 1)
    assert not torch.equal(_raw_sample(model, opts, (B, T, Cc), gt, mask), mixed)
    # ... the setters are sticky: raw dsh_sample calls behind them draw from the row seeds ...
    _lib.check(lib.dsh_sample_set_row_keys(model._h, _u64(keys), B))
    _lib.check(lib.dsh_sample_set_row_seeds(model._h, _u64(seeds), B))
    assert torch.equal(_raw_sample(model, opts, (B, T, Cc), gt, mask), mixed)
    assert torch.equal(_raw_sample(model, opts, (B, T, Cc), gt, mask), mixed)
    # ... refused changes leave them in place (wrong count; more seeds than keys) ...
    assert lib.dsh_sample_set_row_seeds(model._h, _u64(seeds[:2]), 2) == -1 and b"row key" in lib.dsh_last_error()
    assert lib.dsh_sample_set_row_seeds(model._h, _u64(seeds + [1]), 4) == -1
    assert torch.equal(_raw_sample(model, opts, (B, T, Cc), gt, mask), mixed)
    # ... n = 0 clears them: the raw loop is the unseeded one again
    assert lib.dsh_sample_set_row_seeds(model._h, _u64([0]), 0) == 0
    opts = tr.diffusion_ddim_val._opts(0, False, 1, seed)
    assert torch.equal(_raw_sample(model, opts, (B, T, Cc), gt, mask), chain0)
    assert torch.equal(tr.generate_batch(a, p, Cc, cnd, {}, seed=seed, row_keys=keys), plain0)
    assert torch.equal(tr.generate_batch(a, p, Cc, cnd, dict(y), seed=seed, row_keys=keys), chain0)
    # without row keys there is nothing to attach seeds to
    assert lib.dsh_sample_set_row_keys(model._h, _u64([0]), 0) == 0
    assert lib.dsh_sample_set_row_seeds(model._h, _u64(seeds), 3) == -1
    with pytest.raises(ValueError, match="row_keys"):
        tr.generate_batch(a, p, Cc, cnd, {}, seed=seed, row_seeds=seeds)
    model.close()


def test_reopened_slot_starts_from_window_0_and_refusals():
    cfg = get_config("beat")
    tr = DDPMTrainer(sampler_namespace(cfg, jump_n_sample=2), gpu_model("beat", "fp32"))
    size, L = cfg.n_poses, cfg.overlap_len
    N = size + (size - L)                                 # two full windows
    a, h, pid = _features(cfg, N, 150, 4)
    a2, h2, pid2 = _features(cfg, N, 151, 5)

    def run(pool, a_, h_, pid_, key):
        s = pool.open(pid_, key=key)
        pool.feed(s, a_, {"pretrain_aud_feat": h_})
        outs = []
        while True:
            o = pool.step()
            if not o:
                break
            outs.append(o[s])
        slot = pool._sessions[s].slot
        outs.append(pool.close(s))
        return torch.cat(outs, 0), slot
    pool = StreamPool(tr, 1, 31)
    first, slot_a = run(pool, a2, h2, pid2, 1)            # leaves its tail in the only slot
    assert float(pool.tails[slot_a].abs().max()) > 0
    again, slot_b = run(pool, a, h, pid, 2)               # the slot is reused ...
    fresh, _ = run(StreamPool(tr, 1, 31), a, h, pid, 2)
    assert slot_a == slot_b == 0 and torch.equal(again, fresh) and not torch.equal(again, first)      # ... with no trace of the previous tail
    assert torch.equal(fresh, _offline(tr, a, h, pid, 31, 2))
    # refusals
    for over in ({"fix_very_first": True}, {"same_overlap_noisy": True}, {"ddim": False}, {"overlap_len": 0}):
        with pytest.raises(ValueError):
            StreamPool(DDPMTrainer(sampler_namespace(cfg, **over), gpu_model("beat", "fp32")), 2, 0)
    pool = StreamPool(tr, 1, 0)
    s = pool.open(pid)
    with pytest.raises(RuntimeError, match="full"):
        pool.open(pid)
    with pytest.raises(ValueError, match="cond_scale"):
        StreamPool(tr, 1, 0).open(pid, cond_scale=1.5)    # BEAT weights are not classifier-free
    for kw in ({"noise_source": object()}, {"modality": "expression"}):
        with pytest.raises(ValueError, match="noise_source|modality"):
            pool.step(**kw)
        with pytest.raises(ValueError):
            pool.close(s, **kw)
    with pytest.raises(ValueError, match="pretrain_aud_feat"):
        pool.feed(s, a[:3], {})
    pool.feed(s, a[:L], {"pretrain_aud_feat": h[:L]})
    with pytest.raises(ValueError, match="overlap_len"):
        pool.close(s)                                     # 0 < m <= overlap_len and no window yet: refused, the session stays open
    pool.feed(s, a[L:L + 1], {"pretrain_aud_feat": h[L:L + 1]})
    assert tuple(pool.close(s).shape) == (L + 1, cfg.net_dim_pose) and len(pool) == 0
    s = pool.open(pid)
    assert tuple(pool.close(s).shape) == (0, cfg.net_dim_pose)     # nothing fed: nothing owed
    with pytest.raises(KeyError):
        pool.feed(s, a[:3], {"pretrain_aud_feat": h[:3]})
