"""CPU test of audio.plan_chunks: the chunking rule of get_hubert_from_16k_speech_long applied to many utterances at once, against
tests/hubert_ref.py::chunked instrumented with an encode_fn that records what it is handed.  The signal is its own sample index (exact in
float32 below 2^24), so every recorded row names its offset and its length."""
import pytest
import torch

import hubert_ref
from diffsheg_amd import audio

COUNTS = [400, 319_999, 320_000, 320_079, 320_080, 320_479, 320_480, 960_500]
CLIP = hubert_ref.CHUNK + 80


def recorded(n):
    """(full clips as chunk indices, pieces encoded alone as (offset, count), rows returned) of hubert_ref.chunked on n samples"""
    full, alone = [], []

    def encode_fn(x):
        assert x.dim() == 2
        for row in x:
            off, cnt = int(row[0]), int(row.shape[0])
            assert int(row[-1]) == off + cnt - 1
            if x.shape[0] > 1 or cnt == CLIP:
                assert cnt == CLIP and off % hubert_ref.CHUNK == 0
                full.append(off // hubert_ref.CHUNK)
            else:
                alone.append((off, cnt))
        return torch.zeros(x.shape[0], hubert_ref.num_frames(hubert_ref.LARGE, int(x.shape[1])), 1)

    out = hubert_ref.chunked(encode_fn, torch.arange(n, dtype=torch.float32))
    return full, alone, int(out.shape[0])


def test_plan_chunks_is_the_reference_rule_per_utterance():
    full, rest = audio.plan_chunks(COUNTS)
    for u, n in enumerate(COUNTS):
        want_full, want_alone, rows = recorded(n)
        assert [i for v, i in full if v == u] == want_full, f"full clips of {n} samples"
        assert [(off, cnt) for v, off, cnt in rest if v == u] == want_alone, f"remainder of {n} samples"
        assert rows == (n - 80) // 320
        # the rows the plan's pieces give, before the cut / zero-pad, are within one of that count, as the rule demands
        got = 1000 * len(want_full) + sum(hubert_ref.num_frames(hubert_ref.LARGE, cnt) for _, cnt in want_alone)
        assert abs(got - (n - 80) // 320) <= 1
    assert all(cnt >= 400 for _, _, cnt in rest)
    # the cases the list is there for: a clip that fewer than 80 samples follow is encoded alone, shorter than a full one
    assert [(off, cnt) for v, off, cnt in rest if COUNTS[v] == 320_079] == [(0, 320_079)]
    assert [(v, i) for v, i in full if COUNTS[v] == 960_500] == [(7, 0), (7, 1), (7, 2)]


def test_plan_chunks_alone_equals_plan_chunks_in_a_batch():
    full, rest = audio.plan_chunks(COUNTS)
    for u, n in enumerate(COUNTS):
        f1, r1 = audio.plan_chunks([n])
        assert [(u, i) for _, i in f1] == [e for e in full if e[0] == u]
        assert [(u, off, cnt) for _, off, cnt in r1] == [e for e in rest if e[0] == u]


def test_length_groups():
    counts = [5000, 400, 48000, 47000, 36000, 35999, 400, 9000]
    assert audio.length_groups(counts) == [list(range(8))]
    assert audio.length_groups([], 0.75) == [] and audio.length_groups([]) == []
    groups = audio.length_groups(counts, 0.75)
    assert groups == [[2, 3, 4], [5], [7], [0], [1, 6]]                  # 36000 = 0.75 x 48000 still joins; 35999 does not
    assert sorted(k for g in groups for k in g) == list(range(8))
    for g in groups:
        assert min(counts[k] for k in g) >= 0.75 * max(counts[k] for k in g)
    assert audio.length_groups(counts, 0.0) == [list(range(8))]
    assert all(len({counts[k] for k in g}) == 1 for g in audio.length_groups(counts, 1.0))
    with pytest.raises(ValueError):
        audio.length_groups(counts, 1.5)


def test_plan_chunks_refuses_a_signal_below_the_receptive_field():
    with pytest.raises(ValueError):
        audio.plan_chunks([16000, 399])
    with pytest.raises(Exception):
        hubert_ref.chunked(lambda x: torch.zeros(x.shape[0], 1, 1), torch.zeros(399))      # (the rule has nothing to encode either)
