"""The regime of a sampling loop (no GPU): dsh_debug_loop_regime — the function Sampler::run decides through, csrc/loop_regime.h — against
the Python restatement of tests/regime_rules.py, on named rows on both sides of every limit and on a cross product over the boolean
facts; and the table itself is checked for coverage: every field of the regime takes each of its values in at least three rows, and every
term of the rule flips the regime in a pair of rows that differ in that term alone."""
import ctypes as C
import itertools

import pytest

from diffsheg_amd import _lib
from regime_rules import (CACHE_INLINE, CACHE_NONE, CACHE_PREFETCH, CACHE_SUBS, DDIM25, JUMP, PIPE_ROWS, TERMS, _loop_flags, facts, n_streams,
                          regime)

REGIME_FIELDS = ("unsplit", "chains", "forked_evals", "graph", "cache", "inline_ok", "pipe")


class LoopFactsC(C.Structure):
    """dsh_loop_facts"""
    _fields_ = [("struct_size", C.c_uint32)] + [(n, C.c_int32) for n in (
        "kind", "batch", "frames", "channels", "gesture_cols", "modality", "evals", "distinct_levels", "trace", "same_overlap_noisy", "sync",
        "profiling", "cur_split", "no_graph", "level_cache", "level_prefetch", "pipe")] + [(n, C.c_uint64) for n in (
            "graph_rows", "pipe_rows_context", "pipe_rows_sampler")]


class LoopRegimeC(C.Structure):
    """dsh_loop_regime"""
    _fields_ = [("struct_size", C.c_uint32)] + [(n, C.c_int32) for n in REGIME_FIELDS]


def library_regime(f):
    fc, rc = LoopFactsC(struct_size=C.sizeof(LoopFactsC), **f), LoopRegimeC(struct_size=C.sizeof(LoopRegimeC))
    _lib.check(_lib.lib().dsh_debug_loop_regime(C.byref(fc), C.byref(rc)), "dsh_debug_loop_regime")
    return {n: getattr(rc, n) for n in REGIME_FIELDS}


def differing(a, b):
    """The facts in which two rows differ; the schedule's two counts are one fact."""
    return {"schedule" if k in ("evals", "distinct_levels") else k for k in a if a[k] != b[k]}


def R(**kw):
    return dict(dict(unsplit=0, chains=1, forked_evals=0, graph=0, cache=CACHE_NONE, inline_ok=0, pipe=0), **kw)


PIPED = R(unsplit=1, cache=CACHE_PREFETCH, pipe=1)
# name -> (facts, the regime as the rule's author reads it off the shape)
ROWS = {
    # SHOW bf16, T = 88: the graph range (4 048 | 4 136 rows)
    "show 46: graphs": (facts("show", "bf16", 46), R(unsplit=1, graph=1, cache=CACHE_PREFETCH, pipe=1)),
    "show 47: no graphs": (facts("show", "bf16", 47), PIPED),
    # ... one | two sub-batch streams with the pipeline switched off (12 232 | 12 320 rows)
    "show 139 PIPE=0: one stream": (facts("show", "bf16", 139, pipe=0), R(cache=CACHE_PREFETCH)),
    "show 140 PIPE=0: two streams": (facts("show", "bf16", 140, pipe=0), R(chains=2)),
    "show 140: pipeline": (facts("show", "bf16", 140), PIPED),
    # ... the pipeline on one batch | three streams (64 416 | 64 504 rows)
    "show 732: pipeline": (facts("show", "bf16", 732), PIPED),
    "show 733: three streams": (facts("show", "bf16", 733), R(chains=3)),
    # BEAT fp32, T = 34 (4 080 | 4 114 and 8 670 | 8 704 rows)
    "beat 120: graphs": (facts("beat", "fp32", 120), R(unsplit=1, graph=1, cache=CACHE_PREFETCH, pipe=1)),
    "beat 121: no graphs": (facts("beat", "fp32", 121), PIPED),
    "beat 120 PIPE=0: one stream": (facts("beat", "fp32", 120, pipe=0), R(graph=1, cache=CACHE_PREFETCH)),
    "beat 121 PIPE=0: two streams": (facts("beat", "fp32", 121, pipe=0), R(chains=2)),
    "beat 255 PIPE=0: two streams": (facts("beat", "fp32", 255, pipe=0), R(chains=2)),
    "beat 256 PIPE=0: three streams": (facts("beat", "fp32", 256, pipe=0), R(chains=3)),
    "beat 255: pipeline": (facts("beat", "fp32", 255), PIPED),
    "beat 256: pipeline": (facts("beat", "fp32", 256), PIPED),
    # every run that is unsplit without the pipeline
    "show 200: pipeline": (facts("show", "bf16", 200), PIPED),
    "show 200 trace": (facts("show", "bf16", 200, trace=1), R(unsplit=1, cache=CACHE_PREFETCH)),
    "show 200 same_overlap_noisy": (facts("show", "bf16", 200, same_overlap_noisy=1), R(unsplit=1, cache=CACHE_PREFETCH)),
    "show 141: pipeline": (facts("show", "bf16", 141), PIPED),
    "show 141 modality 1": (facts("show", "bf16", 141, modality=1), R(unsplit=1, cache=CACHE_PREFETCH)),
    "show 141 modality 2": (facts("show", "bf16", 141, modality=2), R(unsplit=1, cache=CACHE_PREFETCH)),
    # synchronised windows: unsplit like any loop below the limit; on a context that stays split, one chain of forked evaluations
    "show 200 sync": (facts("show", "bf16", 200, sync=1), PIPED),
    "show 200 sync PIPE=0": (facts("show", "bf16", 200, sync=1, pipe=0), R(forked_evals=1)),
    "show 733 sync": (facts("show", "bf16", 733, sync=1), R(forked_evals=1)),
    "show 46 sync PIPE=0 split by hand": (facts("show", "bf16", 46, sync=1, pipe=0, cur_split=2), R(forked_evals=1)),
    "show 46 PIPE=0 split by hand": (facts("show", "bf16", 46, pipe=0, cur_split=2), R(chains=2)),
    "show 46 PIPE=0": (facts("show", "bf16", 46, pipe=0), R(graph=1, cache=CACHE_PREFETCH)),
    "show 46 sync PIPE=0": (facts("show", "bf16", 46, sync=1, pipe=0), R(graph=1, cache=CACHE_PREFETCH)),
    # profiling: one stream (the context answers 1), nothing on a side stream, no graphs
    "show 46 profiling": (facts("show", "bf16", 46, profiling=1), R()),
    "show 200 profiling": (facts("show", "bf16", 200, profiling=1, cur_split=1), R()),
    "show 46 jump profiling": (facts("show", "bf16", 46, schedule=JUMP, profiling=1), R(cache=CACHE_INLINE, inline_ok=1)),
    "show 200 PIPE=0 profiling, split by hand": (facts("show", "bf16", 200, pipe=0, profiling=1), R()),
    # the switches
    "show 46 LEVEL_CACHE=0": (facts("show", "bf16", 46, level_cache=0), R(graph=1)),
    "show 200 LEVEL_CACHE=0": (facts("show", "bf16", 200, level_cache=0), R(chains=2)),
    "show 46 LEVEL_PREFETCH=0": (facts("show", "bf16", 46, level_prefetch=0), R(graph=1)),
    "show 200 LEVEL_PREFETCH=0": (facts("show", "bf16", 200, level_prefetch=0), R(chains=2)),
    "show 46 NO_GRAPH": (facts("show", "bf16", 46, no_graph=1), PIPED),
    # the single transformer
    "single 46": (facts("single", "bf16", 46), R(graph=1, cache=CACHE_PREFETCH)),
    "single 139": (facts("single", "bf16", 139), R(cache=CACHE_PREFETCH)),
    "single 140": (facts("single", "bf16", 140), R(chains=2)),
    # DDPM: no timestep cache; the pipeline up to the row limit
    "show ddpm 46": (facts("show", "bf16", 46, kind=1), R(unsplit=1, graph=1, pipe=1)),
    "show ddpm 140": (facts("show", "bf16", 140, kind=1), R(unsplit=1, pipe=1)),
    "show ddpm 313": (facts("show", "bf16", 313, kind=1), R(unsplit=1, pipe=1)),
    "show ddpm 140 PIPE=0": (facts("show", "bf16", 140, kind=1, pipe=0), R(chains=2)),
    "show ddpm 313 trace": (facts("show", "bf16", 313, kind=1, trace=1), R(unsplit=1)),
    "show ddpm 313 modality 1": (facts("show", "bf16", 313, kind=1, modality=1), R(unsplit=1)),
    "show ddpm 733": (facts("show", "bf16", 733, kind=1), R(chains=3)),
    # a jump schedule (63 evaluations over 16 levels): the prefetch; the inline cache where there is no prefetch; the sub-batch cache
    "show 47 jump": (facts("show", "bf16", 47, schedule=JUMP), R(unsplit=1, cache=CACHE_PREFETCH, inline_ok=1, pipe=1)),
    "show 47 jump LEVEL_PREFETCH=0": (facts("show", "bf16", 47, schedule=JUMP, level_prefetch=0), R(cache=CACHE_INLINE, inline_ok=1)),
    "show 47 LEVEL_PREFETCH=0": (facts("show", "bf16", 47, level_prefetch=0), R()),
    "beat 120 jump LEVEL_PREFETCH=0": (facts("beat", "fp32", 120, schedule=JUMP, level_prefetch=0), R(graph=1, cache=CACHE_INLINE, inline_ok=1)),
    "show 47 jump LEVEL_CACHE=0": (facts("show", "bf16", 47, schedule=JUMP, level_cache=0), R()),
    "show 140 jump PIPE=0: sub-batch cache": (facts("show", "bf16", 140, schedule=JUMP, pipe=0), R(chains=2, cache=CACHE_SUBS)),
    "show 733 jump: sub-batch cache": (facts("show", "bf16", 733, schedule=JUMP), R(chains=3, cache=CACHE_SUBS)),
    "beat 256 jump PIPE=0: sub-batch cache": (facts("beat", "fp32", 256, schedule=JUMP, pipe=0), R(chains=3, cache=CACHE_SUBS)),
    "show 733 jump LEVEL_CACHE=0": (facts("show", "bf16", 733, schedule=JUMP, level_cache=0), R(chains=3)),
    "show ddpm 733, evals > distinct by hand": (facts("show", "bf16", 733, kind=1, schedule=JUMP), R(chains=3)),
    "show 47 empty schedule": (facts("show", "bf16", 47, schedule=(0, 0)), R(unsplit=1)),
    "show 47 one evaluation": (facts("show", "bf16", 47, schedule=(1, 1)), PIPED),
    # DSH_PIPE_ROWS raised to 200 000 in both readings: the gesture chain's scratch ends at 100 000 rows (1 136 | 1 137 clips)
    "show 1200 PIPE_ROWS=200000": (facts("show", "bf16", 1200, pipe_rows_context=200000, pipe_rows_sampler=200000), R(unsplit=1, cache=CACHE_PREFETCH)),
    "show 1136 PIPE_ROWS=200000": (facts("show", "bf16", 1136, pipe_rows_context=200000, pipe_rows_sampler=200000), PIPED),
    "show 1137 PIPE_ROWS=200000": (facts("show", "bf16", 1137, pipe_rows_context=200000, pipe_rows_sampler=200000), R(unsplit=1, cache=CACHE_PREFETCH)),
    "show ddpm 1136 PIPE_ROWS=200000": (facts("show", "bf16", 1136, kind=1, pipe_rows_context=200000, pipe_rows_sampler=200000), R(unsplit=1, pipe=1)),
    "show ddpm 1137 PIPE_ROWS=200000": (facts("show", "bf16", 1137, kind=1, pipe_rows_context=200000, pipe_rows_sampler=200000), R(unsplit=1)),
    # the two readings of DSH_PIPE_ROWS disagree (the variable changed between the process's first loop and this context)
    "show 200, the context read PIPE_ROWS=100": (facts("show", "bf16", 200, pipe_rows_context=100), R(chains=2)),
    "show 200, the sampler latched PIPE_ROWS=100": (facts("show", "bf16", 200, pipe_rows_sampler=100), R(unsplit=1)),
    "show ddpm 200, the sampler latched PIPE_ROWS=100": (facts("show", "bf16", 200, kind=1, pipe_rows_sampler=100), R(unsplit=1)),
    "show ddpm 200": (facts("show", "bf16", 200, kind=1), R(unsplit=1, pipe=1)),
    # frames * channels no multiple of 4 (87 frames of 231 channels): the sub-batch streams are not used, the context stays split
    "87 x 231, two streams by hand": (facts("show", "bf16", 200, T=87, pipe=0, channels=231, cur_split=2), R()),
    "87 x 232, two streams by hand": (facts("show", "bf16", 200, T=87, pipe=0, cur_split=2), R(chains=2)),
    # the gesture columns: none (one encoder sees all channels), all of them
    "show 200, no gesture columns": (facts("show", "bf16", 200, gesture_cols=0), R(unsplit=1, cache=CACHE_PREFETCH)),
    "show 200, a single transformer": (facts("show", "bf16", 200, gesture_cols=-1), R(chains=2)),
    "show 200, gesture columns only": (facts("show", "bf16", 200, gesture_cols=232), R(unsplit=1, cache=CACHE_PREFETCH)),
}


@pytest.mark.parametrize("name", list(ROWS), ids=lambda v: v.replace(" ", "_"))
def test_named_row(name):
    f, want = ROWS[name]
    assert regime(f) == want, (name, "regime_rules", regime(f), want)
    assert library_regime(f) == want, (name, "dsh_debug_loop_regime", library_regime(f), want)


def test_the_limits_sit_where_the_rows_say():
    """The named rows stand on both sides of each limit at the default switches."""
    assert 46 * 88 <= 4096 < 47 * 88 and 120 * 34 <= 4096 < 121 * 34
    assert (n_streams("bf16", 139, 88), n_streams("bf16", 140, 88), n_streams("bf16", 732, 88), n_streams("bf16", 733, 88)) == (1, 2, 2, 3)
    assert 732 * 88 <= PIPE_ROWS < 733 * 88 and 1136 * 88 <= 100000 < 1137 * 88
    assert (n_streams("fp32", 120, 34), n_streams("fp32", 121, 34), n_streams("fp32", 255, 34), n_streams("fp32", 256, 34)) == (1, 2, 2, 3)
    assert (87 * 231) % 4 != 0 and (87 * 232) % 4 == 0
    assert _loop_flags(733, 88, "bf16", "show", True) == (0, 0, 3) and _loop_flags(200, 88, "bf16", "show", True, trace=True) == (0, 0, 1)


def test_cross_product_over_the_boolean_facts():
    shapes = [("show", "bf16", B) for B in (46, 47, 139, 140, 200, 732, 733, 1200)] + [("beat", "fp32", B) for B in (120, 121, 255, 256)] + \
             [("single", "bf16", 140)]
    flags = ("trace", "same_overlap_noisy", "sync", "profiling", "no_graph", "level_cache", "level_prefetch", "pipe")
    n = 0
    for (model, prec, B), kind, schedule, bits in itertools.product(shapes, (0, 1), (DDIM25, JUMP), itertools.product((0, 1), repeat=len(flags))):
        f = facts(model, prec, B, kind=kind, schedule=schedule, **dict(zip(flags, bits)))
        assert library_regime(f) == regime(f), f
        n += 1
    assert n == len(shapes) * 4 * 256


def test_the_entry_reads_struct_size_bytes_and_refuses_what_it_does_not_know():
    L = _lib.lib()
    f, want = ROWS["show 47 jump"]
    fc, rc = LoopFactsC(struct_size=C.sizeof(LoopFactsC), **f), LoopRegimeC(struct_size=C.sizeof(LoopRegimeC))
    assert L.dsh_debug_loop_regime(None, C.byref(rc)) != 0 and L.dsh_debug_loop_regime(C.byref(fc), None) != 0
    fc.struct_size += 4
    assert L.dsh_debug_loop_regime(C.byref(fc), C.byref(rc)) != 0 and b"struct_size" in L.dsh_last_error()
    fc.struct_size -= 4
    # a caller that knows only the first fields of the result receives those, and nothing is written behind them
    rc = LoopRegimeC(struct_size=LoopRegimeC.graph.offset, pipe=-7)
    assert L.dsh_debug_loop_regime(C.byref(fc), C.byref(rc)) == 0
    assert (rc.unsplit, rc.chains, rc.forked_evals, rc.graph, rc.pipe) == (want["unsplit"], want["chains"], want["forked_evals"], 0, -7)
    # a caller that stops before the switches states them all as 0: no pipeline, no cache, no graphs
    fc.struct_size = LoopFactsC.no_graph.offset
    rc = LoopRegimeC(struct_size=C.sizeof(LoopRegimeC))
    assert L.dsh_debug_loop_regime(C.byref(fc), C.byref(rc)) == 0
    assert {n: getattr(rc, n) for n in REGIME_FIELDS} == R()
    fc.struct_size = C.sizeof(LoopFactsC)
    fc.batch = 0
    assert L.dsh_debug_loop_regime(C.byref(fc), C.byref(rc)) != 0


def test_the_table_covers_every_value_and_every_term():
    table = [f for f, _ in ROWS.values()]
    got = [regime(f) for f in table]
    values = {"unsplit": (0, 1), "chains": (1, 2, 3), "forked_evals": (0, 1), "graph": (0, 1),
              "cache": (CACHE_NONE, CACHE_INLINE, CACHE_PREFETCH, CACHE_SUBS), "inline_ok": (0, 1), "pipe": (0, 1)}
    assert set(values) == set(REGIME_FIELDS)
    for field, vals in values.items():
        for v in vals:
            assert sum(r[field] == v for r in got) >= 3, (field, v)
    # every term flips the regime in a pair of rows that differ in one fact, and in which no other term of the rule changes
    flipped = {}
    for (a, ra), (b, rb) in itertools.combinations(zip(table, got), 2):
        if ra == rb or len(differing(a, b)) != 1:
            continue
        changed = [name for name, term in TERMS.items() if term(a) != term(b)]
        if len(changed) == 1:
            flipped.setdefault(changed[0], []).append((a, b))
    assert set(flipped) == set(TERMS), sorted(set(TERMS) - set(flipped))
    # ... and so do the three conditions the rule derives on the way: sub-batch streams and forked evaluations end the graphs, a DDIM
    # loop without the prefetch has no pipeline
    derived = {"split -> graph": ("show 46 PIPE=0", "show 46 PIPE=0 split by hand"),
               "forked_evals -> graph": ("show 46 sync PIPE=0", "show 46 sync PIPE=0 split by hand"),
               "cache == PREFETCH -> pipe": ("show 47 empty schedule", "show 47 one evaluation")}
    for what, (x, y) in derived.items():
        (fx, rx), (fy, ry) = ROWS[x], ROWS[y]
        field = what.split(" -> ")[1]
        assert len(differing(fx, fy)) == 1 and rx[field] != ry[field], what
