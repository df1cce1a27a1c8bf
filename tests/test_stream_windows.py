"""CPU tests (-m "not gpu") of the live-session window rule (diffsheg_amd.streaming.StreamWindows, the bookkeeping StreamPool uses): a
stream fed in pieces is cut into exactly the windows get_windows / window_lengths cut the whole stream into, with the offline keep
rule ([:step_len] of every window except the last); and the exports of the per-row seeds and the hand-off kernels."""
import inspect
import os
import random

import pytest
import torch

from diffsheg_amd.streaming import StreamPool, StreamWindows
from diffsheg_amd.trainer import DDPMTrainer, get_windows, window_lengths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(88, 10), (34, 4)]          # SHOW, BEAT: (n_poses, overlap_len)


def _offline(N, size, L):
    """(window start, window length, frames kept) of the offline chain on N frames."""
    step = size - L
    lens = window_lengths(N, size, step)
    wins = get_windows(torch.arange(N).view(1, N, 1), size, step)
    assert [int(w.shape[1]) for w in wins] == lens and [int(w[0, 0, 0]) for w in wins] == [i * step for i in range(len(lens))]
    return [(i * step, n, n if i == len(lens) - 1 else step) for i, n in enumerate(lens)]


def _chunks(N, size, rng, mode):
    if mode == "ones":
        return [1] * N
    if mode == "whole":
        return [N]
    out, left = [], N
    while left:
        r = rng.random()
        n = 1 if r < 0.25 else (rng.randint(size + 1, 2 * size + 3) if r < 0.4 else rng.randint(2, size))
        n = min(n, left)
        out.append(n)
        left -= n
    return out


def _stream(N, size, L, chunks, step_every_feed=True):
    """Feed N frames in the given chunks; returns the events [(start, length, emitted)] with close's share folded in, and the checks
    every live caller relies on along the way."""
    w = StreamWindows(size, L)
    events = []

    def drain():
        while w.due():
            events.append(w.take())
            assert w.cursor == len(events) * (size - L) == w.windows * (size - L)
    for n in chunks:
        w.feed(n)
        if step_every_feed:
            drain()
            assert w.pending < size                      # a session that is not due holds fewer than n_poses frames
    drain()
    assert w.fed == N
    kind, start, length, emit = w.close_plan()
    assert w.close_plan() == (kind, start, length, emit)       # (changes nothing)
    if kind == "flush":
        assert events and length == L and start == events[-1][0] + size - L
        s0, n0, e0 = events[-1]
        events[-1] = (s0, n0, e0 + emit)                 # the held-back frames of the last window
    elif kind in ("tail", "short"):
        assert (kind == "short") == (not events) and start == w.cursor and L < length < size
        events.append((start, length, emit))
    else:
        assert kind == "empty" and N == 0
    return events


@pytest.mark.parametrize("size,L", CONFIGS)
def test_streamed_windows_equal_the_offline_windows_for_every_length(size, L):
    rng = random.Random(1000 * size + L)
    for N in range(L + 1, 3 * size + 6):
        want = _offline(N, size, L)
        assert sum(e for _, _, e in want) == N
        for mode in ("ones", "whole", "random", "random", "random"):
            chunks = _chunks(N, size, rng, mode)
            assert sum(chunks) == N
            for every in (True, False):
                got = _stream(N, size, L, chunks, every)
                assert got == want, (N, mode, chunks, got, want)
    # chunks of 1 and chunks longer than a window were both among the random ones
    seen = [c for N in (3 * size + 5,) for _ in range(20) for c in _chunks(N, size, rng, "random")]
    assert 1 in seen and any(c > size for c in seen)


@pytest.mark.parametrize("size,L", CONFIGS)
def test_close_cases_that_must_raise(size, L):
    """No window yet and 0 < m <= overlap_len: a window has to be longer than the frames the hand-off pins."""
    for N in range(1, L + 1):
        for chunks in ([N], [1] * N):
            w = StreamWindows(size, L)
            for n in chunks:
                w.feed(n)
            assert not w.due()
            with pytest.raises(ValueError, match="overlap_len"):
                w.close_plan()
            # nothing changed: the stream can be fed on and closed then
            w.feed(L + 1 - N)
            assert w.close_plan() == ("short", 0, L + 1, L + 1)
    w = StreamWindows(size, L)
    assert w.close_plan() == ("empty", 0, 0, 0)
    w.feed(size)
    with pytest.raises(ValueError, match="due"):
        w.close_plan()                                   # a due window is taken first
    assert w.take() == (0, size, size - L) and w.close_plan() == ("flush", size - L, L, L)
    with pytest.raises(ValueError):
        w.take()
    with pytest.raises(ValueError):
        w.feed(0)
    for bad in ((10, 0), (10, 10), (10, 11)):
        with pytest.raises(ValueError):
            StreamWindows(*bad)


def test_window_index_is_the_offline_window_index():
    """The Philox key of a window is hash(seed, window index): the streamed chain numbers its windows as the offline loop does."""
    size, L = 34, 4
    w = StreamWindows(size, L)
    w.feed(2 * 30 + 4 + 17)
    idx = []
    while w.due():
        idx.append(w.windows)
        w.take()
    assert idx == [0, 1] and w.windows == 2 and w.close_plan()[0] == "tail"       # the tail is window 2


def test_stream_exports_are_declared_and_bound():
    from diffsheg_amd import _lib
    from diffsheg_amd.diffusion import GaussianDiffusion
    header = open(os.path.join(ROOT, "include", "diffsheg_hip.h")).read()
    for name in ("dsh_sample_set_row_seeds", "dsh_op_philox_randn_rows_seeded", "dsh_op_philox_randn_rows_ragged_seeded",
                 "dsh_op_chain_handoff", "dsh_op_chain_save_tail"):
        assert name in _lib.SYMBOLS, name
        assert f"int {name}(" in header, name
        assert hasattr(_lib.lib(), name)
    assert "row_seeds" in inspect.signature(GaussianDiffusion._run).parameters
    assert "row_seeds" in (DDPMTrainer.generate_batch.__doc__ or "")
    for meth in ("open", "feed", "step", "close", "close_many"):
        assert callable(getattr(StreamPool, meth))
