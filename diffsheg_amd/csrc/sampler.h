// Sampling-loop driver (host) — see sampler.hip for the reference citations.
#pragma once
#include <string>
#include <vector>

#include "denoiser.h"
#include "loop_regime.h"

namespace dsh {

struct DiffusionTables {
    std::vector<double> betas, ac, ac_prev, ac_next, c1, c2, post_var, post_logvar, coef1, coef2;   // ac_next[k] = ac[k + 1], last entry 0
    std::vector<int> tmap;   // spaced index -> original timestep
};
void build_tables(const std::vector<double>& betas, DiffusionTables& t);
std::vector<double> linear_betas(int n);
int make_tables(int steps, int respacing, DiffusionTables& out, std::string& err);
// The tables of a free subset of the base process: kept = the original timesteps, strictly ascending, each in [0, steps), at least one.
// beta'_k = 1 - ac[kept_k] / ac[kept_{k-1}], tmap = kept.  make_tables(steps, K > 0) is this with the 'ddimK' stride's list.
int make_tables_kept(int steps, const std::vector<int>& kept, DiffusionTables& out, std::string& err);
int stride_timesteps(int steps, int respacing, std::vector<int>& kept, std::string& err);      // the 'ddimK' list
// Out-painting start t_T of a subset that is no 'ddimK' stride: 1 + the first level whose alphas_cumprod is at or below that of level 14 of
// the ddim25 tables of the same base process (where the reference starts a masked window); the top level if there is none.  0 (= the
// reference's index rule 15 / int(0.6 K)) for an empty list and for a list that is the stride of its own length.
int masked_start_level(int steps, const std::vector<int>& kept, std::string& err);
// DPM-Solver++(2M) coefficients of spaced level k, fp64: with ab = ac[k], abp = ac_prev[k], lambda(a) = log(a / (1 - a)) / 2,
// h = lambda(abp) - lambda(ab):  A = sqrt((1 - abp) / (1 - ab)), Bc = -sqrt(abp) expm1(-h), G = h / (2 (lambda(ab) - lambda(ac[k + 1]))).
// G is 0 at the levels that have no second-order step (k = 0, where h is infinite, and the top level).
void solver_coeffs(const DiffusionTables& t, int k, double& A, double& Bc, double& G);
enum Solver { SOLVER_DDIM = 0, SOLVER_DPM2M = 1 };
std::vector<int> jump_schedule(int respacing, int jump_length, int jump_n_sample);
// the same walk from t_T = start_level (an edit restarts the RePaint schedule from its own level); 0: the built-in 15 / 0.6 * respacing
std::vector<int> jump_schedule_from(int respacing, int jump_length, int jump_n_sample, int start_level);

struct SamplerOpts {
    int kind = 0, diffusion_steps = 1000, respacing = 25, jump_length = 3, jump_n_sample = 5, overlap_len = 10,
        add_blend = 1, no_resample = 0, no_repaint = 0, clip_denoised = 0, noise_mode = 0;
    uint64_t seed = 0;
    int same_overlap_noisy = 0, clip_idx = 0;     // gaussian_diffusion.py:1040-1060: window index inside a chain
    float eta = 0.f;                              // DDIM eta (gaussian_diffusion.py:1011-1032)
};
// STEP_REVERSE: one step of the DDIM reverse ODE (ddim_reverse_sample, gaussian_diffusion.py:1068-1104): level k -> k + 1, no draw
enum StepKind { STEP_DDIM = 0, STEP_UNDO = 1, STEP_DDPM = 2, STEP_REVERSE = 3 };
struct SamplerStep { StepKind kind; int level; };

// Everything one loop needs from its caller.  The Sampler keeps none of it between calls.
//   init         0 x_T is drawn (draw 0), 1 x is given at the schedule's first level, 2 x holds x0 and is noised to that level with draw 0
//   start_level  K (DDIM, 1 .. respacing; 0: the whole schedule): the plain schedule is levels K-1 .. 0, the mask-present one
//                jump_schedule_from(K); x enters at level K - 1 (an edit of an existing motion: init 1 or 2)
//   invert_to    > 0: the reverse loop (DDIM inversion, ddim_reverse_sample, gaussian_diffusion.py:1068-1104): x, a clean motion at
//                invert_from 0 or a state at that level, is carried up the reverse ODE through levels invert_from .. invert_to - 1 in
//                place; no draws (init, the noise fields, the solver and the row keys are not read), eta = 0 only, no mask
//   kept         the free timestep subset the DDIM loops and the reverse loop run on instead of the 'ddimK' stride (empty: the stride):
//                strictly ascending, its length o.respacing, every entry in [0, o.diffusion_steps).  The counts depend on its length and,
//                mask-present, on masked_start_level() only
//   solver       SOLVER_DPM2M: a DDIM step at level k whose previous executed step of the run was the DDIM step at level k + 1, k != 0, is
//                the second-order DPM-Solver++(2M) update; every other step (the first of a run, the one after an undo step, the last) is
//                the DDIM update bit for bit.  Draws are those of the DDIM loop.  eta = 0 only, no same_overlap_noisy, no DDPM loop
//   tail_blend   windows pinned at both ends (in-betweening / seam repair): the DDIM step's cross-fade also runs, mirrored, on the last
//                overlap_len frames (sampler_kernels.hip); false = the reference's head-only fade
//   row_keys     Philox mode: one key per batch row (empty: one stream for the whole batch).  A chain keyed by its global id draws the same
//                noise whatever batch / rank it is sampled in (sharded long-audio path)
//   row_seeds    beside the row keys, one per key: row b draws from the key row_seeds[b] in place of o.seed (every draw of the run: x_T, the
//                steps' randn_like, the RePaint blend's gt noise, the undo steps, the eta scratch; main chain and gesture-side twin alike),
//                so rows of one batch may stand at different windows of their chains
//   trace        (nullable) [steps, n]: the sample after every step
//   sync_left    synchronised window batches (empty: off, nothing is launched): one entry per batch row, the row that holds
//                this row's first sync_len frames as its last sync_len valid frames (-1: none).  Behind every DDIM step each chain
//                reconciles the shared frames of its columns (launch_window_sync); trace rows are taken after it.  Needs init 1 (the
//                caller's x_T holds ONE noise value per stream frame), eta = 0, no mask; the run is one chain (check_run())
//   guide        soft constraints: every denoise step of the forward loops is the guided form of its kernel
//                (sampler_kernels.hip); undo steps, draws and the evaluations are untouched.  Not for the reverse loop.
// The guidance of a run: target / weight [B, T, C] and vel / acc [C] on the device (each may be null), stated with the shape the caller
// built them for (check_run() compares it with the context's); level_scale: one factor per spaced level of the run (DDIM: respacing, DDPM:
// diffusion_steps entries; empty: 1 everywhere).  A level whose factor is 0 runs the unguided kernel.
struct Guidance {
    bool on = false;
    const float *target = nullptr, *weight = nullptr, *vel = nullptr, *acc = nullptr;
    int space = 0;                       // GuideSpace (dsh_kernels.h)
    int batch = 0, frames = 0, channels = 0;
    std::vector<float> level_scale;
};
struct RunSpec {
    SamplerOpts o;
    int init = 0;
    float* x = nullptr; const float* gt = nullptr; const uint8_t* mask = nullptr; bool masked = false;
    const float* noise_stack = nullptr; int64_t n_draws = 0;
    float* trace = nullptr;
    int start_level = 0, invert_from = 0, invert_to = 0;
    std::vector<int> kept;
    int solver = SOLVER_DDIM;
    bool tail_blend = false;
    std::vector<uint64_t> row_keys, row_seeds;
    Guidance guide;
    std::vector<int32_t> sync_left; int sync_len = 0;
};
// what check_run() needs of the conditioned context (lengths: the ragged batch's per-clip frame counts on the host, or null)
struct RunShape { int batch, frames, channels, gesture_cols, modality; const int32_t* lengths; };
// Every refusal of a run, on the host, with no GPU call and no state: 0, or -1 with the reason in err.  shape null: what can be said without
// a conditioned context (the counting path); else also the pointers and what depends on the batch (the noise stack's length is run()'s to
// check, against the schedule it plans next).
int check_run(const RunSpec& s, const RunShape* shape, std::string& err);
// draws (Gaussian tensors the loop consumes; 0 for the reverse loop) and steps (rows of a trace) of a run; either may be null.  -1 with
// set_last_error() on what check_run(s, null) refuses.
int sampler_count(const RunSpec& s, int64_t* draws, int64_t* steps);

class Sampler {
  public:
    Sampler(hipStream_t s, int channels_) : st(s), channels(channels_) {}
    ~Sampler();
    Profiler* prof = nullptr;
    // the forward loops and the reverse loop (s.invert_to > 0); -1 before any state changes on what check_run() refuses
    int run(DenoiserContext* den, const RunSpec& s);

  private:
    // One set of the device buffers a chain works in: the noise scratch of a step's two draws, the per-step scalars an evaluation reads
    // (timestep, the two input scales, the level's cache slot: one per batch row, 8 level words) and the hipGraphs of one evaluation, one per
    // timestep-cache mode (denoiser.h, EvalMode: plain, compute + save level, restore level).  Replayed in launch-bound (small-batch /
    // window-chain) runs: all pointers are fixed for a run, only the scalars' contents change between steps.
    struct ChainBufs {
        float *nz1 = nullptr, *nz_eta = nullptr, *c1 = nullptr, *c2 = nullptr;
        int64_t *t = nullptr, *lvl = nullptr;
        hipGraph_t graph[3] = {}; hipGraphExec_t graph_exec[3] = {};
    };
    // One stream that advances some columns of some rows through every step of a run.  Three ways of filling it (run()):
    //   whole batch            the context's denoiser and stream, all clips, the active modality's columns, bufs[0]
    //   sub-batch i            sub_get(i)'s instance and stream, its clips, the same columns, bufs[0] at its clips' offset (lvl: word i)
    //   pipelined loop E / G   the context's denoiser and stream on the expression columns with bufs[0] / the gesture-side twin and its
    //                          stream on the gesture columns, one step behind, with bufs[1]
    struct Chain {
        DenoiserInstance* inst; hipStream_t s;   // the instance that evaluates it; null: the run's context does (whole batch, E)
        int b0, nb; size_t off, cnt;        // clips [b0, b0 + nb) = elements [off, off + cnt) of x / eps / gt / mask / the noise scratch
        int c_lo, c_hi;                     // the columns its updates write (0, 0: all)
        float *nz1, *nz_eta;                // full-size scratch (the chain uses its element range): the gt / undo / DDPM draw, the eta != 0 draw
        int64_t* t; float *c1, *c2; int64_t* lvl;      // its rows of the per-step scalars, its level word
        ChainBufs* own;                     // the set these come from: holds its evaluation graphs
    };
    // (sampler.hip) one run()'s arguments, constants, regime (loop_regime.h) and chains; what one step's launches share
    struct Run; struct StepConsts;
    // run() = argument checks, the schedule, the regime from loop_facts(), then these in order; finish() joins the chains whatever loop() returned
    LoopFacts loop_facts(Run& r, const RunSpec& s) const;
    int ensure(size_t n, int B, bool want_hist);
    int prepare(Run& r, const RunSpec& s);
    int make_chains(Run& r);
    int loop(Run& r);
    int finish(Run& r, int rc);
    // loop() = x_T, setup(), then per step: evaluate(), and update() of every chain (pipelined: E, gesture_follow(), G)
    int setup(Run& r);
    StepConsts step_consts(Run& r, const SamplerStep& sp);
    int noise_for(const Run& r, int64_t idx, const Chain& c, float* scratch, const float** out);
    int evaluate(Run& r, const StepConsts& sc);
    int eval_step(const Run& r, const Chain& c, int n_eval, bool use_graph, int mode);
    int gesture_follow(Run& r, const StepConsts& sc);
    int update(Run& r, const Chain& c, const StepConsts& sc);
    int ddim_update(Run& r, const Chain& c, const StepConsts& sc);
    int ddpm_update(Run& r, const Chain& c, const StepConsts& sc);
    bool guide_for(const Run& r, const Chain& c, const StepConsts& sc, GuideArgs& g) const;
    static void drop_graphs(ChainBufs& b);
    void drop_graph();                     // every chain's
    bool replayed() const { return bufs[0].graph_exec[0] || bufs[0].graph_exec[1] || bufs[0].graph_exec[2]; }
    hipStream_t st;
    int channels;
    std::vector<void*> pool;              // ensure()'s allocations
    size_t cap_n = 0; int cap_b = 0;
    float* eps = nullptr;
    float* hist = nullptr; size_t cap_hist = 0;     // SOLVER_DPM2M: x0 of the previous step, [B, T, C] addressed like x (grown with cap_n on demand)
    // [0] the whole batch / the sub-batches / the expression chain; [1] the gesture chain of the pipelined loop, its noise scratch sized for
    // the batches that loop serves (cap_n2).  bufs[0].nz_eta is grown on demand (cap_eta): Philox runs with eta != 0 only.
    ChainBufs bufs[2];
    size_t cap_n2 = 0, cap_eta = 0;
    DiffusionTables tb; int tb_steps = -1, tb_resp = -1; std::vector<int> tb_kept;    // cache key: (steps, respacing, subset)
    // the device copies of a run's row keys / row seeds with what they hold (host): a caller that keeps its keys pays one upload, not one per run
    uint64_t* row_keys = nullptr; int cap_row_keys = 0; std::vector<uint64_t> row_keys_held;
    uint64_t* row_seeds = nullptr; int cap_row_seeds = 0; std::vector<uint64_t> row_seeds_held;
    template <typename V> int upload_rows(const std::vector<V>& host, V*& dev, int& cap, std::vector<V>& held);
    // ... and of a run's sync_left, cached the same way; window_sync(): one chain's reconciliation behind its DDIM step
    int32_t* sync_left = nullptr; int cap_sync = 0; std::vector<int32_t> sync_left_held;
    int window_sync(Run& r, const Chain& c);
    int init_x(Run& r);
    // --same_overlap_noisy: the noisy tail x[..., -L:, :] saved after every DDIM step, one slot per spaced level; persists
    // across sample() calls like the reference's self.saved_noisy_tail (the dict the next window receives IS this object)
    float* tails = nullptr; float* tail_tmp = nullptr; size_t tails_blc = 0; int tails_levels = 0;
    // pipelined small-batch loop (denoiser.h: set_part / pipe_begin)
    hipEvent_t ev_pE = nullptr, ev_pC = nullptr, ev_pG = nullptr;       // E_k done / E_k's expression estimate copied / gesture chain done
    // free-running sub-batch streams of large batches (run(): one fork before the loop, one join after it)
    hipEvent_t ev_fork = nullptr;
    std::vector<hipEvent_t> ev_sub;      // [2 i] = "sub-batch i has queued its first launches" (stagger), [2 i + 1] = "sub-batch i done"
};

}  // namespace dsh
