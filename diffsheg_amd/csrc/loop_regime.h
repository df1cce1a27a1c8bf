// The regime of a sampling loop, decided in ONE pure host function: no HIP call, no environment read, no state.  Sampler::run fills
// LoopFacts once per run (the only place of the sampling path that reads the regime switches) and calls loop_regime() before anything
// changes in the context or on the device; dsh_debug_loop_regime hands the same function to tests that have no GPU
// (tests/test_loop_regime_cpu.py pins its truth table against the Python restatement in tests/regime_rules.py).
#pragma once
#include <cstddef>

namespace dsh {

// timestep cache of a loop (denoiser.h, EvalMode): none, filled inline at a level's first use, filled ahead by the side-stream prefetch,
// or inline per sub-batch stream
enum LevelCache { CACHE_NONE, CACHE_INLINE, CACHE_PREFETCH, CACHE_SUBS };

// Everything the regime depends on, as plain values.
struct LoopFacts {
    int kind = 0;                               // 0 DDIM (the reverse loop included), 1 DDPM
    int batch = 0, frames = 0, channels = 0;
    int gesture_cols = -1;                      // -1: a single transformer
    int modality = 0;
    int evals = 0, distinct = 0;                // DDIM: evaluations of the schedule, distinct levels among them
    bool trace = false, same_overlap_noisy = false, sync = false, profiling = false;      // sync: synchronised windows on
    int cur_split = 1;                          // what the context's sub_count() answers before the loop
    // the switches, as their readers see them
    size_t graph_rows = 0; bool no_graph = false;              // DSH_GRAPH_ROWS, DSH_NO_GRAPH
    long level_cache = 1, level_prefetch = 1, pipe = 1;        // DSH_LEVEL_CACHE, DSH_LEVEL_PREFETCH, DSH_PIPE
    size_t pipe_rows_context = 0, pipe_rows_sampler = 0;       // DSH_PIPE_ROWS as the context read it when it was created / as the process latched it
};

struct LoopRegime {
    bool unsplit = false;                // the context conditions the batch as ONE batch for this loop (and remembers the shape)
    int chains = 1;                      // 1: the whole batch on the context stream; n > 1: n free-running sub-batch streams
    bool forked_evals = false;           // one chain whose evaluations fork and join the context's sub-batch streams (synchronised windows)
    bool graph = false;                  // evaluations replayed from hipGraphs
    LevelCache cache = CACHE_NONE;
    bool inline_ok = false;              // a prefetch that fails at run time falls back to the inline cache (the schedule revisits levels)
    bool pipe = false;                   // the two encoders' chains on two streams
    bool split() const { return chains > 1; }
};

// The two-encoder pipeline exists at all: it restores every head from the slots a side-stream prefetch run fills, so all three switches
// must be on; a single transformer has one encoder; a profiled batch runs on one stream.  (The one piece of the policy the context
// evaluates itself — for the sticky shape, at set_condition time, when no run exists.)
inline bool pipe_available(long pipe, long level_prefetch, long level_cache, int gesture_cols, bool profiling) {
    return pipe != 0 && level_prefetch != 0 && level_cache != 0 && gesture_cols >= 0 && !profiling;
}

// Runs that are unsplit WITHOUT the pipeline: `unsplit` asks only whether the pipeline exists and the batch is below the row limit, so a
// mid-size loop with a per-step trace, with same_overlap_noisy or with a partial modality runs as one batch on one stream (ADVICE.md
// finding 1 measures what the first two cost against two sub-batch streams).  Existing tests pin all of them
// (test_mid_size_loop_is_bit_identical_pipelined_split_and_traced, test_gpu_modality.py, test_gpu_synchronised_windows.py), so changing it
// is a behaviour change — with this header a two-line one: move those terms from `pipe` into `unsplit`.
inline LoopRegime loop_regime(const LoopFacts& f) {
    LoopRegime r;
    const size_t rows = (size_t)f.batch * f.frames, n = rows * f.channels, row_n = (size_t)f.frames * f.channels;
    const int g = f.gesture_cols;
    r.unsplit = pipe_available(f.pipe, f.level_prefetch, f.level_cache, g, f.profiling) && rows <= f.pipe_rows_context;
    const int ns = r.unsplit ? 1 : f.cur_split;
    // sub-batch streams run free through all steps: never while profiling events are recorded, never with synchronised windows
    // (neighbouring rows must not live in different streams), and the Philox addressing needs whole quads per clip
    r.chains = (f.profiling || f.sync || !(ns > 1 && row_n % 4 == 0)) ? 1 : ns;
    r.forked_evals = f.sync && ns > 1;
    // graphs only where launches dominate (a few thousand token rows); sub-batch streams and forked evaluations run eagerly
    r.graph = rows <= f.graph_rows && !f.profiling && !f.no_graph && !r.split() && !r.forked_evals;
    // (the side-stream head and the two-stream encoder pipeline also pay above the graph range, up to where batches are split)
    const bool small_pf = rows <= f.pipe_rows_sampler, cache_on = f.level_cache != 0;
    // the gesture chain's scratch serves batches below the three-stream range only (100 000 values per channel)
    const bool pipe_fits = f.modality == 0 && !f.trace && n <= (size_t)100000 * f.channels && g > 0 && g < f.channels && f.pipe != 0;
    if (r.split()) {
        // sub-batch streams: the inline timestep cache for schedules that revisit levels, else plain evaluations
        if (f.kind == 0 && f.evals > f.distinct && cache_on) r.cache = CACHE_SUBS;
    } else if (ns != 1) {
        // one chain on a context that stays split: plain evaluations (the cache and the pipeline are single-stream features)
    } else if (f.kind == 0 && (rows <= f.graph_rows || small_pf)) {
        // side-stream prefetch of every scheduled level (also pays for schedules without repeats); else the inline cache, worth it when
        // the schedule revisits levels (out-painting jump schedule: 63 evaluations over 16 levels)
        r.inline_ok = f.evals > f.distinct && cache_on;
        r.cache = (cache_on && !f.profiling && f.evals > 0 && f.level_prefetch != 0) ? CACHE_PREFETCH : r.inline_ok ? CACHE_INLINE : CACHE_NONE;
        // every evaluation restores its head from the slots the prefetch run fills; no per-step trace of the whole sample, no saved noisy
        // tails (both need all channels of a step at once)
        r.pipe = pipe_fits && r.cache == CACHE_PREFETCH && !f.same_overlap_noisy;
    } else if (f.kind == 1 && small_pf) {
        // DDPM loops have no timestep cache (every level is visited once, 1000 of them): each chain computes its own head
        r.pipe = pipe_fits;
    }
    return r;
}

}  // namespace dsh
