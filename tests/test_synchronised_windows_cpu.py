"""Synchronised window batches, host side: the plan that turns streams into ONE batch of windows, the keep rule that
stitches the batch back, and the torch restatement of the scheme (tests/synchronised_ref.py) — under it both copies of every shared
frame are equal after every step, which is what the GPU tests then ask of the native loop."""
import pytest
import torch

from diffsheg_amd.trainer import get_windows, stitch_synchronised, synchronised_window_plan, window_lengths
from synchronised_ref import copies_equal, max_copy_gap, synchronised_loop, window_sync

N_POSES, L = 12, 3
STEP = N_POSES - L


def _used_both_sides(plan):
    lefts = {p for p in plan["left"] if p >= 0}
    return [b for b, p in enumerate(plan["left"]) if p >= 0 and b in lefts]


@pytest.mark.parametrize("n", range(1, 61))
def test_plan_of_one_stream_is_the_chain_s_window_list(n):
    plan = synchronised_window_plan([n], N_POSES, L)
    idx = torch.arange(n)[None]
    wins = get_windows(idx, N_POSES, STEP)
    assert plan["lengths"] == window_lengths(n, N_POSES, STEP) == [int(w.shape[1]) for w in wins]
    assert plan["start"] == [int(w[0, 0]) for w in wins]
    assert plan["stream"] == [0] * len(wins) and plan["window"] == list(range(len(wins))) and plan["ranges"] == [(0, len(wins))]
    assert plan["left"] == [-1] + list(range(len(wins) - 1))
    assert plan["frames"] == max(plan["lengths"]) or (len(wins) >= 7 and plan["frames"] == 11)
    # the kernel's conditions: left is injective, a row used at both ends holds 2 L frames, a tail row more than L
    used = [p for p in plan["left"] if p >= 0]
    assert len(set(used)) == len(used) and all(p != b for b, p in enumerate(plan["left"]))
    assert all(plan["lengths"][b] >= 2 * L for b in _used_both_sides(plan))
    assert all(plan["lengths"][b] >= L for b in used)
    if len(wins) > 1:
        assert plan["lengths"][-1] > L
    # every shared frame is the same stream frame in both rows
    for b, p in enumerate(plan["left"]):
        if p >= 0:
            assert plan["start"][p] + plan["lengths"][p] - L == plan["start"][b]
    # cut and stitch: the stream comes back
    rows = torch.full((len(wins), plan["frames"]), -1)
    for r, w in enumerate(wins):
        rows[r, :w.shape[1]] = w[0]
    (back,) = stitch_synchronised(rows, plan, L)
    assert torch.equal(back, idx[0])


@pytest.mark.parametrize("frames", [(40, 21), (5, 40), (30, 12, 47), (21, 2, 21), (12, 13)])
def test_plan_of_several_streams(frames):
    plan = synchronised_window_plan(list(frames), N_POSES, L)
    B = len(plan["stream"])
    # the row ranges partition the batch, stream-major
    assert plan["ranges"][0][0] == 0 and plan["ranges"][-1][1] == B
    assert all(plan["ranges"][s][1] == plan["ranges"][s + 1][0] for s in range(len(frames) - 1))
    for s, (lo, hi) in enumerate(plan["ranges"]):
        assert plan["stream"][lo:hi] == [s] * (hi - lo)
        assert plan["lengths"][lo:hi] == window_lengths(frames[s], N_POSES, STEP)
        assert plan["start"][lo:hi] == [i * STEP for i in range(hi - lo)]
        assert plan["left"][lo:hi] == [-1] + list(range(lo, hi - 1))        # no left crosses a stream
    used = [p for p in plan["left"] if p >= 0]
    assert len(set(used)) == len(used)
    assert plan["frames"] == max(plan["lengths"]) or (B >= 7 and plan["frames"] == 11)
    # cut by the plan, stitch by the keep rule
    streams = [torch.arange(n) + 1000 * s for s, n in enumerate(frames)]
    rows = torch.full((B, plan["frames"]), -1)
    for r in range(B):
        n = plan["lengths"][r]
        rows[r, :n] = streams[plan["stream"][r]][plan["start"][r]:plan["start"][r] + n]
    for got, want in zip(stitch_synchronised(rows, plan, L), streams):
        assert torch.equal(got, want)


def test_plan_pads_a_large_batch_of_short_windows():
    plan = synchronised_window_plan([4] * 7, N_POSES, L)
    assert plan["lengths"] == [4] * 7 and plan["left"] == [-1] * 7 and plan["frames"] == 11
    assert synchronised_window_plan([4] * 6, N_POSES, L)["frames"] == 4


def test_plan_refusals():
    for bad_l in (0, -1):
        with pytest.raises(ValueError, match="overlap_len >= 1"):
            synchronised_window_plan([40], N_POSES, bad_l)
    with pytest.raises(ValueError, match="2 \\* overlap_len <= n_poses"):
        synchronised_window_plan([40], 12, 7)
    synchronised_window_plan([40], 12, 6)                # 2 L == n_poses is the limit
    for bad in ([], [0], [12, -3]):
        with pytest.raises(ValueError, match="at least one"):
            synchronised_window_plan(bad, N_POSES, L)


# ---- the scheme itself, restated in torch -----------------------------------------------------------------------------------------
def _stub_eps(M):
    """eps of a row depends on EVERY frame of the row (a frame mean, like attention would) and on the level"""
    def f(x, lvl):
        return torch.tanh(x @ M + x.mean(dim=1, keepdim=True) * (0.3 + 0.01 * lvl))
    return f


def test_sync_formula_restated():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(5, 12, 7, generator=g)
    left, lens = [-1, 0, 1, -1, 3], [12, 12, 7, 12, 11]
    for Lc in (1, 2, 3):
        for cols in ((0, 0), (3, 7), (0, 3)):
            y = window_sync(x, left, Lc, lens, *cols)
            cs = slice(None) if cols == (0, 0) else slice(*cols)
            w = torch.linspace(0, 1, Lc)
            touched = torch.zeros_like(x, dtype=torch.bool)
            for b, p in enumerate(left):
                if p < 0:
                    continue
                for j in range(Lc):
                    a, r = x[p, lens[p] - Lc + j, cs], x[b, j, cs]
                    v = a * (1 - w[j]) + r * w[j]
                    assert torch.equal(y[p, lens[p] - Lc + j, cs], v) and torch.equal(y[b, j, cs], v)
                    touched[p, lens[p] - Lc + j, cs] = True
                    touched[b, j, cs] = True
            assert torch.equal(y[~touched], x[~touched])
            # the left window is trusted at its interior end of the overlap, the right one at its own
            if Lc > 1 and cols == (0, 0):
                assert torch.equal(y[0, lens[0] - Lc], x[0, lens[0] - Lc]) and torch.equal(y[1, Lc - 1], x[1, Lc - 1])
    assert torch.equal(window_sync(x, [-1] * 5, 3, lens), x)


@pytest.mark.parametrize("frames", [(40,), (33, 12, 26)])
def test_restated_loop_keeps_the_copies_equal_after_every_step(frames):
    C = 6
    plan = synchronised_window_plan(list(frames), N_POSES, L)
    B, T = len(plan["stream"]), plan["frames"]
    g = torch.Generator().manual_seed(11)
    M = torch.randn(C, C, generator=g) * 0.4
    z = [torch.randn(n, C, generator=g) for n in frames]            # ONE noise value per stream frame
    x_T = torch.zeros(B, T, C)
    for r in range(B):
        n = plan["lengths"][r]
        x_T[r, :n] = z[plan["stream"][r]][plan["start"][r]:plan["start"][r] + n]
    lens = plan["lengths"]
    assert copies_equal(x_T, plan["left"], L, lens)
    trace = synchronised_loop(_stub_eps(M), x_T, plan["left"], L, lens)
    assert trace.shape[0] == 25 and torch.isfinite(trace).all()
    for i in range(25):
        assert copies_equal(trace[i], plan["left"], L, lens), i
    if B > len(frames):
        # ... and the reconciliation is what does it: without it the copies part at the first step
        free = synchronised_loop(_stub_eps(M), x_T, plan["left"], L, lens, sync=False)
        assert max_copy_gap(free[0], plan["left"], L, lens) > 1e-3
        # windows that started from different noise are NOT kept equal by later steps alone: equality needs the shared start
        other = x_T.clone()
        b = next(b for b, p in enumerate(plan["left"]) if p >= 0)
        other[b, :L] += 1.0
        assert not copies_equal(other, plan["left"], L, lens)
    # the stitched stream has every frame once
    out = stitch_synchronised(trace[-1], plan, L)
    assert [int(o.shape[0]) for o in out] == list(frames)
