"""The regime of a sampling loop, restated in plain Python (no library, no GPU): which loops run unsplit, on how many sub-batch streams,
from hipGraphs, with which timestep cache and on the two-encoder pipeline.  The library decides in csrc/loop_regime.h (`loop_regime`); this
module is written from the rule, not from that code.  tests/test_loop_regime_cpu.py compares the two through dsh_debug_loop_regime on
both sides of every limit; tests/test_gpu_dispatch_sweep.py compares what a real loop reports with `_loop_flags`."""

SPLIT = {"bf16": (12288, 21500), "fp32": (4096, 2900)}                 # denoiser_context.hip: (min rows, rows per stream)
SPLIT["bf16x3"] = SPLIT["fp32"]                                        # precision "bf16x3" is fp32 storage: the same stream rules
GRAPH_ROWS, PIPE_ROWS = 4096, 64499                                    # switches.h: DSH_GRAPH_ROWS, DSH_PIPE_ROWS
PIPE_SCRATCH_ROWS = 100000                                             # sampler.hip ensure(): the gesture chain's scratch, values per channel
CACHE_NONE, CACHE_INLINE, CACHE_PREFETCH, CACHE_SUBS = 0, 1, 2, 3      # loop_regime.h LevelCache
# model -> (frames per window, channels, gesture columns; -1: a single transformer)
MODELS = {"show": (88, 232, 129), "beat": (34, 192, 141), "single": (88, 232, -1)}
DDIM25, JUMP, DDPM = (25, 25), (63, 16), (0, 0)                        # (evaluations, distinct levels): plain ddim25, the out-painting jump schedule


def n_streams(prec, B, T):
    """DenoiserContext: want_split (default DSH_DUAL = 3, profiler off)."""
    rows = B * T
    min_rows, per_stream = SPLIT[prec]
    if rows < min_rows:
        return 1
    return min(3, max(2, rows // per_stream), B)


def facts(model, prec, B, T=None, kind=0, schedule=None, cur_split=None, **over):
    """The facts of a loop of B clips on `model` at the default switches; cur_split: what a fresh condition gives (n_streams)."""
    frames, channels, gcols = MODELS[model]
    T = frames if T is None else T
    evals, distinct = schedule if schedule is not None else (DDIM25 if kind == 0 else DDPM)
    f = dict(kind=kind, batch=B, frames=T, channels=channels, gesture_cols=gcols, modality=0, evals=evals, distinct_levels=distinct,
             trace=0, same_overlap_noisy=0, sync=0, profiling=0, cur_split=n_streams(prec, B, T) if cur_split is None else cur_split,
             no_graph=0, level_cache=1, level_prefetch=1, pipe=1, graph_rows=GRAPH_ROWS, pipe_rows_context=PIPE_ROWS, pipe_rows_sampler=PIPE_ROWS)
    assert not set(over) - set(f), set(over) - set(f)
    f.update(over)
    return f


# every condition the rule is built from, as a predicate of the facts
TERMS = {
    "PIPE != 0": lambda f: f["pipe"] != 0,
    "LEVEL_PREFETCH != 0": lambda f: f["level_prefetch"] != 0,
    "LEVEL_CACHE != 0": lambda f: f["level_cache"] != 0,
    "g >= 0": lambda f: f["gesture_cols"] >= 0,
    "profiling": lambda f: bool(f["profiling"]),
    "rows <= pipe_rows(context)": lambda f: f["batch"] * f["frames"] <= f["pipe_rows_context"],
    "cur_split > 1": lambda f: f["cur_split"] > 1,
    "sync": lambda f: bool(f["sync"]),
    "row_n % 4 == 0": lambda f: f["frames"] * f["channels"] % 4 == 0,
    "rows <= GRAPH_ROWS": lambda f: f["batch"] * f["frames"] <= f["graph_rows"],
    "NO_GRAPH": lambda f: bool(f["no_graph"]),
    "DDIM": lambda f: f["kind"] == 0,
    "rows <= pipe_rows(sampler)": lambda f: f["batch"] * f["frames"] <= f["pipe_rows_sampler"],
    "evals > distinct": lambda f: f["evals"] > f["distinct_levels"],
    "evals > 0": lambda f: f["evals"] > 0,
    "modality == 0": lambda f: f["modality"] == 0,
    "trace": lambda f: bool(f["trace"]),
    "same_overlap_noisy": lambda f: bool(f["same_overlap_noisy"]),
    "n <= 100000 C": lambda f: f["batch"] * f["frames"] <= PIPE_SCRATCH_ROWS,
    "g > 0": lambda f: f["gesture_cols"] > 0,
    "g < C": lambda f: f["gesture_cols"] < f["channels"],
}


def regime(f):
    """The regime of the loop with facts `f` (a dict as `facts` builds it): dict of unsplit, chains, forked_evals, graph, cache, inline_ok, pipe."""
    t = {name: term(f) for name, term in TERMS.items()}
    pipe_available = t["PIPE != 0"] and t["LEVEL_PREFETCH != 0"] and t["LEVEL_CACHE != 0"] and t["g >= 0"] and not t["profiling"]
    unsplit = pipe_available and t["rows <= pipe_rows(context)"]
    ns = 1 if unsplit else f["cur_split"]
    chains = ns if (not t["profiling"] and not t["sync"] and ns > 1 and t["row_n % 4 == 0"]) else 1
    split = chains > 1
    forked_evals = t["sync"] and ns > 1
    graph = t["rows <= GRAPH_ROWS"] and not t["profiling"] and not t["NO_GRAPH"] and not split and not forked_evals
    small_pf, cache_on = t["rows <= pipe_rows(sampler)"], t["LEVEL_CACHE != 0"]
    two_chains = t["modality == 0"] and not t["trace"] and t["n <= 100000 C"] and t["g > 0"] and t["g < C"] and t["PIPE != 0"]
    cache, inline_ok, pipe = CACHE_NONE, False, False
    if t["DDIM"] and not split and (t["rows <= GRAPH_ROWS"] or small_pf) and ns == 1:
        inline_ok = t["evals > distinct"] and cache_on
        if cache_on and not t["profiling"] and t["evals > 0"] and t["LEVEL_PREFETCH != 0"]:
            cache = CACHE_PREFETCH
        elif inline_ok:
            cache = CACHE_INLINE
        pipe = two_chains and cache == CACHE_PREFETCH and not t["same_overlap_noisy"]
    elif not t["DDIM"] and not split and small_pf and ns == 1:
        pipe = two_chains
    elif split and t["DDIM"] and t["evals > distinct"] and cache_on:
        cache = CACHE_SUBS
    return dict(unsplit=int(unsplit), chains=chains, forked_evals=int(forked_evals), graph=int(graph), cache=cache, inline_ok=int(inline_ok), pipe=int(pipe))


def _loop_flags(B, T, prec, kind, pipe_env, ddim=True, trace=False, **over):
    """(graphs, pipeline, sub-batch streams) of a plain loop (loop_regime.h) on a freshly conditioned context: model `kind`, DSH_PIPE on / off."""
    r = regime(facts(kind, prec, B, T, kind=0 if ddim else 1, pipe=int(bool(pipe_env)), trace=int(bool(trace)), **over))
    return r["graph"], r["pipe"], r["chains"]
