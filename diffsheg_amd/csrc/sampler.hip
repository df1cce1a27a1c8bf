// Host side of the sampling loops: coefficient tables, respacing, the RePaint jump schedule and
// the DDIM / harmonize / DDPM drivers.  Everything is enqueued on the context stream; there are
// no host<->device syncs inside a loop (the reference syncs several times per step:
// `True in mask`, `noise_weight[0,0,0] < 0.2`, per-step H2D table copies — SURVEY.md §3.1).
//
//   tables        GaussianDiffusion.__init__      models/gaussian_diffusion.py:334-390 (fp64)
//   respacing     space_timesteps/SpacedDiffusion models/respace.py:7-34,68-82
//   schedule      get_schedule_jump_cjm_ddim      models/scheduler.py:178-208
//   loops         ddim_sample_loop(+harmonize)    models/gaussian_diffusion.py:1106-1278
//                 p_sample_loop_progressive       models/gaussian_diffusion.py:923-974
// Not in the reference: free timestep subsets (make_tables_kept, masked_start_level) and the DPM-Solver++(2M) update of the DDIM
// loops (solver_coeffs, the order rule in step_consts(), the x0 history) — sampler.h, DESIGN.md 4.18.
#include "sampler.h"

#include <math.h>
#include <stdlib.h>

namespace dsh {

void build_tables(const std::vector<double>& betas, DiffusionTables& t) {
    const size_t n = betas.size();
    t.betas = betas;
    t.ac.resize(n); t.ac_prev.resize(n); t.ac_next.resize(n); t.c1.resize(n); t.c2.resize(n); t.post_var.resize(n);
    t.post_logvar.resize(n); t.coef1.resize(n); t.coef2.resize(n);
    double cp = 1.0;
    for (size_t i = 0; i < n; ++i) {
        t.ac_prev[i] = cp;
        cp *= (1.0 - betas[i]);
        t.ac[i] = cp;
    }
    for (size_t i = 0; i < n; ++i) t.ac_next[i] = i + 1 < n ? t.ac[i + 1] : 0.0;      // alphas_cumprod_next (:347)
    for (size_t i = 0; i < n; ++i) {
        t.c1[i] = sqrt(1.0 / t.ac[i]);
        t.c2[i] = sqrt(1.0 / t.ac[i] - 1.0);
        t.post_var[i] = betas[i] * (1.0 - t.ac_prev[i]) / (1.0 - t.ac[i]);
        t.coef1[i] = betas[i] * sqrt(t.ac_prev[i]) / (1.0 - t.ac[i]);
        t.coef2[i] = (1.0 - t.ac_prev[i]) * sqrt(1.0 - betas[i]) / (1.0 - t.ac[i]);
    }
    for (size_t i = 0; i < n; ++i) t.post_logvar[i] = log(t.post_var[i == 0 ? (n > 1 ? 1 : 0) : i]);
}

std::vector<double> linear_betas(int n) {
    // np.linspace(scale*1e-4, scale*0.02, n): start + i*step with step = (stop-start)/(n-1), last = stop
    const double scale = 1000.0 / n, b0 = scale * 1e-4, b1 = scale * 0.02;
    std::vector<double> b(n);
    const double step = n > 1 ? (b1 - b0) / (n - 1) : 0.0;
    for (int i = 0; i < n; ++i) b[i] = b0 + i * step;
    if (n > 1) b[n - 1] = b1;
    return b;
}

int make_tables(int steps, int respacing, DiffusionTables& out, std::string& err) {
    if (steps < 2) { err = "diffusion_steps must be >= 2"; return -1; }
    DiffusionTables base;
    build_tables(linear_betas(steps), base);
    if (respacing <= 0) {
        out = base;
        out.tmap.resize(steps);
        for (int i = 0; i < steps; ++i) out.tmap[i] = i;
        return 0;
    }
    std::vector<int> kept;
    if (stride_timesteps(steps, respacing, kept, err)) return -1;
    return make_tables_kept(steps, kept, out, err);
}

int stride_timesteps(int steps, int respacing, std::vector<int>& kept, std::string& err) {
    // 'ddimK': first integer stride whose range(0, steps, stride) has exactly K entries
    int stride = 0;
    for (int s = 1; s < steps; ++s)
        if ((steps + s - 1) / s == respacing) { stride = s; break; }
    if (!stride) { err = "cannot create exactly " + std::to_string(respacing) + " steps with an integer stride"; return -1; }
    kept.clear();
    for (int i = 0; i < steps; i += stride) kept.push_back(i);
    return 0;
}

int make_tables_kept(int steps, const std::vector<int>& kept, DiffusionTables& out, std::string& err) {
    if (steps < 2) { err = "diffusion_steps must be >= 2"; return -1; }
    if (kept.empty()) { err = "a timestep subset needs at least one entry"; return -1; }
    for (size_t i = 0; i < kept.size(); ++i) {
        if (kept[i] < 0 || kept[i] >= steps) { err = "timestep subset: entry outside [0, diffusion_steps)"; return -1; }
        if (i > 0 && kept[i] <= kept[i - 1]) { err = "timestep subset: entries must be strictly ascending"; return -1; }
    }
    DiffusionTables base;
    build_tables(linear_betas(steps), base);
    std::vector<double> nb;
    double last = 1.0;
    for (int i : kept) {
        nb.push_back(1.0 - base.ac[i] / last);
        last = base.ac[i];
    }
    build_tables(nb, out);
    out.tmap = kept;
    return 0;
}

int masked_start_level(int steps, const std::vector<int>& kept, std::string& err) {
    if (kept.empty()) return 0;
    std::vector<int> strided; std::string ignored;
    if (stride_timesteps(steps, (int)kept.size(), strided, ignored) == 0 && strided == kept) return 0;
    DiffusionTables sub, ref;
    if (make_tables_kept(steps, kept, sub, err)) return -1;
    if (make_tables(steps, 25, ref, err)) return -1;
    const double at = ref.ac[14];
    for (size_t k = 0; k < sub.ac.size(); ++k) if (sub.ac[k] <= at) return (int)k + 1;
    return (int)sub.ac.size();
}

static double half_logsnr(double a) { return 0.5 * log(a / (1.0 - a)); }
void solver_coeffs(const DiffusionTables& t, int k, double& A, double& Bc, double& G) {
    const double ab = t.ac[k], abp = t.ac_prev[k];
    const double h = half_logsnr(abp) - half_logsnr(ab);               // (k = 0: abp = 1, h = +inf, A = 0, Bc = 1)
    A = sqrt((1.0 - abp) / (1.0 - ab));
    Bc = -sqrt(abp) * expm1(-h);
    G = (k == 0 || k + 1 >= (int)t.ac.size()) ? 0.0 : h / (2.0 * (half_logsnr(ab) - half_logsnr(t.ac[k + 1])));
}

std::vector<int> jump_schedule(int respacing, int jump_length, int jump_n_sample) {
    return jump_schedule_from(respacing, jump_length, jump_n_sample, 0);
}
std::vector<int> jump_schedule_from(int respacing, int jump_length, int jump_n_sample, int start_level) {
    const int t_T = start_level > 0 ? start_level : respacing == 25 ? 15 : (int)(respacing * 0.6);
    std::vector<int> jumps(t_T > 0 ? t_T : 1, 0);
    if (jump_length > 0)
        for (int j = 0; j < t_T - jump_length; j += jump_length) jumps[j] = jump_n_sample - 1;
    std::vector<int> ts;
    int t = t_T;
    while (t >= 1) {
        t -= 1;
        ts.push_back(t);
        if (t < (int)jumps.size() && jumps[t] > 0) {
            jumps[t] -= 1;
            for (int i = 0; i < jump_length; ++i) { t += 1; ts.push_back(t); }
        }
    }
    ts.push_back(-1);
    return ts;
}

// ------------------------------------------------------------------------------------------------
// Every refusal of a run (sampler.h).  The order is part of the interface: callers read the first reason.
int check_run(const RunSpec& s, const RunShape* sh, std::string& err) {
#define RUN_REQUIRE(cond, msg) do { if (!(cond)) { err = (msg); return -1; } } while (0)
    const SamplerOpts& o = s.o;
    const bool reverse = s.invert_to > 0, son = o.same_overlap_noisy != 0, philox = o.noise_mode == 1;
    RUN_REQUIRE(reverse || (s.init >= 0 && s.init <= 2), "unknown init mode");
    RUN_REQUIRE(reverse || s.init != 2 || o.kind == 0, "init mode 2 (x holds x0) exists for the DDIM loops only");
    RUN_REQUIRE(o.noise_mode == 0 || philox, "unknown noise mode");
    // the timestep subset
    for (size_t i = 0; i < s.kept.size(); ++i) {
        RUN_REQUIRE(s.kept[i] >= 0, "timestep subset: entry outside [0, diffusion_steps)");
        RUN_REQUIRE(i == 0 || s.kept[i] > s.kept[i - 1], "timestep subset: entries must be strictly ascending");
    }
    if (!s.kept.empty()) {
        RUN_REQUIRE(o.kind == 0, "a timestep subset exists for the DDIM loops only");
        RUN_REQUIRE((int)s.kept.size() == o.respacing, "the timestep subset's length differs from opts.respacing");
        RUN_REQUIRE(s.kept.back() < o.diffusion_steps, "timestep subset: entry outside [0, diffusion_steps)");
    }
    // a start level, the reverse loop
    if (s.start_level != 0 || s.invert_to != 0) {
        RUN_REQUIRE(o.kind == 0, "a start level / the reverse loop exist for the DDIM loops only");
        RUN_REQUIRE(s.start_level >= 0 && s.start_level <= o.respacing, "start level outside 1 .. respacing");
        RUN_REQUIRE(s.invert_to >= 0 && s.invert_to <= o.respacing, "inversion level outside 1 .. respacing");
    }
    RUN_REQUIRE(s.start_level == 0 || (!son && !s.tail_blend), "a start level exists for the DDIM loops only, without same_overlap_noisy and the tail blend");
    RUN_REQUIRE(reverse ? (s.invert_from >= 0 && s.invert_from < s.invert_to) : s.invert_from == 0, "the reverse loop needs 0 <= from_level < to_level");
    if (reverse) {
        RUN_REQUIRE(!s.masked && s.start_level == 0, "the reverse loop takes no mask and no start level");
        RUN_REQUIRE(o.eta == 0.f, "the reverse ODE exists for the DDIM loops at eta = 0 only");
        RUN_REQUIRE(!son && !s.tail_blend, "same_overlap_noisy and the tail blend do not apply to the reverse loop");
    }
    RUN_REQUIRE(o.kind == 0 || o.kind == 1, "unknown sampler kind");
    RUN_REQUIRE(s.solver == SOLVER_DDIM || s.solver == SOLVER_DPM2M, "unknown solver (0 ddim, 1 dpm2m)");
    if (s.solver == SOLVER_DPM2M && !reverse) {                   // (the reverse ODE stays first-order whatever the solver)
        RUN_REQUIRE(o.kind == 0, "the dpm2m solver exists for the DDIM loops only");
        RUN_REQUIRE(o.eta == 0.f, "the dpm2m solver is deterministic: eta must be 0");
        RUN_REQUIRE(!son, "the dpm2m solver does not keep the saved noisy tails of same_overlap_noisy");
    }
    RUN_REQUIRE(!(s.tail_blend && son), "tail_blend with same_overlap_noisy: the saved noisy tails describe a window chain, not a window pinned at both ends");
    RUN_REQUIRE(s.row_seeds.empty() || s.row_seeds.size() == s.row_keys.size(), "row seeds need the row keys, and one seed per row key");
    // soft constraints
    const Guidance& gd = s.guide;
    if (gd.on) {
        RUN_REQUIRE(!reverse, "guidance does not apply to the reverse loop (DDIM inversion)");
        RUN_REQUIRE(gd.space == GUIDE_XT || gd.space == GUIDE_X0, "unknown guidance space (0 x_t, 1 x0)");
        RUN_REQUIRE(gd.level_scale.empty() || (int64_t)gd.level_scale.size() == (o.kind == 1 ? o.diffusion_steps : o.respacing),
                    "guidance: the level scales need one entry per level of the run (DDIM: respacing, DDPM: diffusion_steps)");
    }
    // synchronised window batches: whatever would put per-window noise into the shared frames is refused
    const bool sync = !s.sync_left.empty();
    if (sync) {
        RUN_REQUIRE(!reverse, "synchronised windows do not apply to the reverse loop");
        RUN_REQUIRE(o.kind == 0, "synchronised windows exist for the DDIM loops only (the DDPM loop draws per-window noise at every step)");
        RUN_REQUIRE(o.eta == 0.f, "synchronised windows are deterministic: eta must be 0");
        RUN_REQUIRE(!s.masked, "synchronised windows take no mask (the RePaint schedule's undo steps draw per-window noise)");
        RUN_REQUIRE(!son, "synchronised windows with same_overlap_noisy: nothing is handed from window to window");
        RUN_REQUIRE(!s.tail_blend, "synchronised windows with the tail blend: there is no mask to blend under");
        RUN_REQUIRE(s.start_level == 0, "synchronised windows run the whole schedule: no start level");
        RUN_REQUIRE(philox, "synchronised windows take no noise stack: the caller supplies x_T with one noise value per stream frame");
        RUN_REQUIRE(s.init == 1, "synchronised windows need init = 1: the caller supplies x_T with one noise value per stream frame");
        RUN_REQUIRE(s.sync_len >= 1, "synchronised windows need sync_len >= 1");
    }
    if (!sh) return 0;
    // what depends on the conditioned context
    RUN_REQUIRE(s.x != nullptr, "null sample buffer");
    RUN_REQUIRE(!s.masked || (s.gt && s.mask), "masked sampling needs gt and mask");
    RUN_REQUIRE(!(s.masked && o.kind == 1), "mask-present DDPM (p_sample_loop_progressive_harmonize) is not supported");
    RUN_REQUIRE(!s.tail_blend || (o.overlap_len >= 0 && 2 * (int64_t)o.overlap_len <= sh->frames), "tail_blend: the head and the tail fade overlap (2 * overlap_len > frames)");
    RUN_REQUIRE(sh->modality == 0 || (sh->gesture_cols > 0 && sh->gesture_cols < sh->channels), "a partial modality needs the UniDiffuser's two encoders");
    RUN_REQUIRE(sh->modality == 0 || !son, "same_overlap_noisy with a partial modality: the saved noisy tails describe all channels");
    // (both address the last overlap_len frames of the PADDED window, which a short clip does not reach)
    RUN_REQUIRE(!sh->lengths || (!son && !s.tail_blend), "per-clip lengths cannot be combined with same_overlap_noisy or the tail blend");
    // (the reverse loop draws nothing: row keys do not concern it)
    if (!s.row_keys.empty() && philox && !reverse) {
        RUN_REQUIRE((int)s.row_keys.size() == sh->batch && ((int64_t)sh->frames * sh->channels) % 4 == 0,
                    "row keys were set for a different batch size (or frames*channels is not a multiple of 4)");
        for (int b = 0; sh->lengths && b < sh->batch; ++b)
            RUN_REQUIRE(((int64_t)sh->lengths[b] * sh->channels) % 4 == 0, "row keys on a ragged batch: length * channels must be a multiple of 4 for every clip");
    }
    if (sync) {
        RUN_REQUIRE((int)s.sync_left.size() == sh->batch, "sync_left was built for a different batch size");
        if (check_window_sync(s.sync_left.data(), sh->lengths, sh->batch, sh->frames, s.sync_len, err)) return -1;
    }
    if (gd.on) {
        RUN_REQUIRE(!(gd.target || gd.weight) || (gd.batch == sh->batch && gd.frames == sh->frames && gd.channels == sh->channels),
                    "guidance: target / weight were built for a different [batch, frames, channels] than the condition's");
        RUN_REQUIRE(!(gd.vel || gd.acc) || gd.channels == sh->channels, "guidance: vel / acc were built for a different channel count than the condition's");
    }
    return 0;
#undef RUN_REQUIRE
}

// The schedule of a spec check_run() has passed.  A start level: the DDIM schedules begin at level start_level - 1; a mask-present schedule on
// a free subset without one begins at masked_start_level().
static int plan_steps(const RunSpec& s, std::vector<SamplerStep>& steps, std::string& err) {
    const SamplerOpts& o = s.o;
    steps.clear();
    if (s.invert_to > 0) {
        for (int k = s.invert_from; k < s.invert_to; ++k) steps.push_back({STEP_REVERSE, k});
    } else if (o.kind == 1) {  // DDPM ancestral, full chain
        for (int t = o.diffusion_steps - 1; t >= 0; --t) steps.push_back({STEP_DDPM, t});
    } else if (s.masked && !o.no_repaint) {
        int start = s.start_level;
        if (start == 0 && !s.kept.empty()) {
            start = masked_start_level(o.diffusion_steps, s.kept, err);
            if (start < 0) return -1;
        }
        const std::vector<int> times = o.no_resample ? jump_schedule_from(o.respacing, 1, 1, start)
                                                     : jump_schedule_from(o.respacing, o.jump_length, o.jump_n_sample, start);
        for (size_t i = 0; i + 1 < times.size(); ++i) {
            const int t_last = times[i], t_cur = times[i + 1];
            if (t_last < 0 || t_last >= o.respacing) { err = "jump schedule leaves the spaced range"; return -1; }
            steps.push_back({t_cur < t_last ? STEP_DDIM : STEP_UNDO, t_last});
        }
    } else {
        for (int k = (s.start_level > 0 ? s.start_level : o.respacing) - 1; k >= 0; --k) steps.push_back({STEP_DDIM, k});
    }
    return 0;
}

static int64_t count_draws(const RunSpec& s, const std::vector<SamplerStep>& steps) {
    if (s.invert_to > 0) return 0;
    int64_t n = s.init == 1 ? 0 : 1;                                                      // x_T, or the q_sample noise of init 2
    const bool tail_gt = s.masked && s.o.same_overlap_noisy && s.o.clip_idx > 0;          // that branch draws no gt noise
    for (const auto& sp : steps) n += (sp.kind == STEP_DDIM) ? ((s.masked && !tail_gt) ? 2 : 1) : 1;
    return n;
}

int sampler_count(const RunSpec& s, int64_t* draws, int64_t* steps) {
    std::vector<SamplerStep> plan; std::string err;
    if (check_run(s, nullptr, err) || plan_steps(s, plan, err)) { set_last_error(err); return -1; }
    if (draws) *draws = count_draws(s, plan);
    if (steps) *steps = (int64_t)plan.size();
    return 0;
}

// One run()'s arguments, what is derived from them once, its chains and the loop's running state; the parts of run() share it by reference.
struct Sampler::Run {
    DenoiserContext* den; const SamplerOpts& o; float* x; int init; const float* gt; const uint8_t* mask; bool masked;
    const float* noise_stack; float* trace; bool tail_blend;
    int B = 0; size_t n = 0, row_n = 0;                  // clips, values, values per clip
    int mod = 0, gcols = 0, w_lo = 0, w_hi = 0;          // modality, gesture columns, the active column window (0, 0: all)
    const int* len_d = nullptr;                          // ragged batch: per-clip frame counts (device)
    std::vector<SamplerStep> steps;
    std::vector<int> order;                              // DDIM: the schedule's levels in first-use order
    LoopRegime want;                                     // the regime (loop_regime.h), decided before anything is queued
    bool per_row = false; const uint64_t* seeds_d = nullptr; uint64_t quads = 0;      // Philox addressing
    bool son = false, tail_gt = false; size_t blc = 0;   // --same_overlap_noisy state
    std::vector<Chain> chains;                           // the whole batch, or its sub-batches
    Chain E{}, G{};                                      // pipelined loop (piped): chains[0] on the expression columns, the twin on the gesture columns
    LevelCache cache = CACHE_NONE; bool piped = false;   // what setup() obtained of the regime
    std::vector<char> level_seen;
    std::vector<int64_t> tv; int lag = 0;                // level -> model timestep; DSH_DUAL_LAG
    size_t pf_next = 0;                                  // order[0 .. pf_next) have been handed to the prefetch stream
    int64_t draw = 0, step_idx = 0; int n_eval = 0;
    bool dpm = false; int last_ddim_level = -1;          // SOLVER_DPM2M; level of the previous executed step if it was a DDIM step, else -1
    const Guidance* guide = nullptr;                     // soft constraints of the run (null: none)
    const int32_t* sync_d = nullptr; int sync_len = 0;   // synchronised windows: the left neighbours (device; null: off), the overlap
    int64_t next_draw() { return draw++; }               // draw index: advanced once per draw, whatever the regime
};

// what the launches of one step share
struct Sampler::StepConsts {
    StepKind kind; int k; int eval_idx;                  // spaced level; index of the step's evaluation in the run (-1: undo step)
    int64_t t; float c1, c2;                             // model timestep and the input scales of the evaluation
    int64_t idx, idx2;                                   // draws: the step's own N(0,1) (undo / DDPM noise, DDIM randn_like); the noised gt's (-1: none)
    float undo_a, undo_b, coef1, coef2;                  // undo step; DDPM step (with sigma)
    float sqrt_ab_prev, sqrt_1m_ab_prev, coef_eps, sigma;
    float sqrt_1m_ab = 0.f, post_var = 0.f;              // guided steps: sqrt(1 - abar) (condition_score), the posterior variance (condition_mean)
    bool second = false; float sA = 0.f, sBc = 0.f, sG = 0.f;      // SOLVER_DPM2M: a second-order step and its coefficients
};

Sampler::~Sampler() {
    drop_graph();
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    for (hipEvent_t e : {ev_pE, ev_pC, ev_pG}) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_sub) (void)hipEventDestroy(e);
    for (void* p : pool) (void)hipFree(p);
    for (void* p : {(void*)row_keys, (void*)row_seeds, (void*)sync_left, (void*)tails, (void*)tail_tmp, (void*)bufs[0].nz_eta, (void*)hist}) if (p) (void)hipFree(p);
}

// a run's row keys / row seeds on the device: uploaded (and waited for: `host` is the caller's) unless the buffer holds exactly these values
template <typename V>
int Sampler::upload_rows(const std::vector<V>& host, V*& dev, int& cap, std::vector<V>& held) {
    if (host == held) return 0;
    held.clear();
    if ((int)host.size() > cap) { if (int e = grow_device_buffer(dev, cap, host.size(), st)) return e; }
    DSH_HIP_CHECK(hipMemcpyAsync(dev, host.data(), host.size() * sizeof(V), hipMemcpyHostToDevice, st));
    DSH_HIP_CHECK(hipStreamSynchronize(st));
    held = host;
    return 0;
}

void Sampler::drop_graphs(ChainBufs& b) {
    for (int m = 0; m < 3; ++m) {
        if (b.graph_exec[m]) { (void)hipGraphExecDestroy(b.graph_exec[m]); b.graph_exec[m] = nullptr; }
        if (b.graph[m]) { (void)hipGraphDestroy(b.graph[m]); b.graph[m] = nullptr; }
    }
}
void Sampler::drop_graph() { drop_graphs(bufs[1]); drop_graphs(bufs[0]); }

// One denoiser evaluation eps = model(x, t, c1, c2) of a chain, on its stream.  At small batch an eval is ~170 launches of a few
// microseconds each, i.e. launch / dependency bound: the first eval of a run executes eagerly (also warms one-time
// kernel attribute setup), later ones are stream-captured into a hipGraph once per cache mode and replayed.
// All pointers (x, the chain's scalars, eps, the denoiser workspace and its timestep-cache slots) are fixed for
// the duration of a run; only the CONTENTS of the scalars change between steps, so one graph per mode serves every step.
// A failed capture or instantiation drops the chain's graphs and evaluates eagerly.
int Sampler::eval_step(const Run& r, const Chain& c, int n_eval, bool use_graph, int mode) {
    float* xc = r.x + c.off; float* ec = eps + c.off;      // (a chain without an instance is the whole batch, evaluated by the context)
    auto eager = [&]() -> int { return c.inst ? c.inst->eval_level(xc, c.t, c.c1, c.c2, ec, mode, c.lvl) : r.den->eval_level(xc, c.t, c.c1, c.c2, ec, mode, c.lvl); };
    if (!use_graph || n_eval == 0) return eager();
    ChainBufs& g = *c.own;
    if (!g.graph_exec[mode]) {
        if (hipStreamBeginCapture(c.s, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); return eager(); }
        const int rc = eager();
        hipError_t e = hipStreamEndCapture(c.s, &g.graph[mode]);
        const bool captured = rc == 0 && e == hipSuccess && g.graph[mode] != nullptr;
        if (!captured || hipGraphInstantiate(&g.graph_exec[mode], g.graph[mode], nullptr, nullptr, 0) != hipSuccess) {
            (void)hipGetLastError();
            drop_graphs(g);
            return rc != 0 ? rc : eager();
        }
    }
    DSH_HIP_CHECK(hipGraphLaunch(g.graph_exec[mode], c.s));
    return 0;
}

int Sampler::ensure(size_t n, int B, bool want_hist) {
    if (want_hist && cap_hist < std::max(n, cap_n)) {
        DSH_HIP_CHECK(hipStreamSynchronize(st));
        if (hist) (void)hipFree(hist);
        hist = nullptr; cap_hist = 0;
        DSH_HIP_CHECK(hipMalloc((void**)&hist, std::max(n, cap_n) * sizeof(float)));
        cap_hist = std::max(n, cap_n);
    }
    if (n <= cap_n && B <= cap_b) return 0;
    DSH_HIP_CHECK(hipStreamSynchronize(st));
    for (void* p : pool) (void)hipFree(p);
    pool.clear();
    cap_n = std::max(n, cap_n); cap_b = std::max(B, cap_b);
    auto alloc = [&](void** p, size_t bytes) -> int {
        DSH_HIP_CHECK(hipMalloc(p, bytes)); pool.push_back(*p); return 0; };
    auto scalars = [&](ChainBufs& b) -> int {
        if (int e = alloc((void**)&b.t, cap_b * sizeof(int64_t))) return e;
        if (int e = alloc((void**)&b.c1, cap_b * sizeof(float))) return e;
        if (int e = alloc((void**)&b.c2, cap_b * sizeof(float))) return e;
        return alloc((void**)&b.lvl, 8 * sizeof(int64_t));                       // one per sub-batch stream
    };
    if (int e = alloc((void**)&eps, cap_n * sizeof(float))) return e;
    if (int e = alloc((void**)&bufs[0].nz1, cap_n * sizeof(float))) return e;
    if (int e = scalars(bufs[0])) return e;
    // (pipelined loop: the gesture chain's own scalars and noise scratch, sized for the batches that loop serves — below the sub-batch split's
    //  three-stream range — whatever larger batch this context has also sampled)
    cap_n2 = std::min(cap_n, (size_t)100000 * channels);
    if (int e = alloc((void**)&bufs[1].nz1, cap_n2 * sizeof(float))) return e;
    if (int e = alloc((void**)&bufs[1].nz_eta, cap_n2 * sizeof(float))) return e;
    return scalars(bufs[1]);
}

// what run() needs beside its spec: the coefficient tables, the buffers, the noise addressing, the saved noisy tails
int Sampler::prepare(Run& r, const RunSpec& s) {
    const SamplerOpts& o = r.o;
    const int B = r.B; const size_t n = r.n;
    const bool reverse = s.invert_to > 0;
    std::string err;
    // tables are cached per (steps, respacing, subset)
    const int resp = o.kind == 1 ? 0 : o.respacing;
    if (tb_steps != o.diffusion_steps || tb_resp != resp || tb_kept != s.kept) {
        tb_steps = tb_resp = -1;
        if (s.kept.empty() ? make_tables(o.diffusion_steps, resp, tb, err) : make_tables_kept(o.diffusion_steps, s.kept, tb, err)) { set_last_error(err); return -1; }
        tb_steps = o.diffusion_steps; tb_resp = resp; tb_kept = s.kept;
    }
    r.dpm = s.solver == SOLVER_DPM2M && !reverse;
    if (int e = ensure(n, B, r.dpm)) return e;
    if (o.kind == 0 && o.eta != 0.f && o.noise_mode == 1 && cap_eta < n) { if (int e = grow_device_buffer(bufs[0].nz_eta, cap_eta, n, st)) return e; }
    // (the reverse loop draws nothing: row keys do not concern it; check_run(): one key per batch row, one seed per key)
    r.per_row = !reverse && o.noise_mode == 1 && !s.row_keys.empty();
    if (r.per_row) { if (int e = upload_rows(s.row_keys, row_keys, cap_row_keys, row_keys_held)) return e; }
    if (r.per_row && !s.row_seeds.empty()) {
        if (int e = upload_rows(s.row_seeds, row_seeds, cap_row_seeds, row_seeds_held)) return e;
        r.seeds_d = row_seeds;
    }
    r.quads = r.per_row ? (n / B) / 4 : (n + 3) / 4;
    if (!s.sync_left.empty()) {
        if (int e = upload_rows(s.sync_left, sync_left, cap_sync, sync_left_held)) return e;
        r.sync_d = sync_left; r.sync_len = s.sync_len;
    }
    // --same_overlap_noisy state
    r.blc = (size_t)B * o.overlap_len * channels;
    r.son = o.same_overlap_noisy != 0 && o.kind == 0;
    if (r.son) {
        DSH_REQUIRE(o.overlap_len > 0 && o.overlap_len <= r.den->frames(), "same_overlap_noisy needs 0 < overlap_len <= frames");
        if (tails_blc != r.blc || tails_levels != o.respacing) {
            DSH_REQUIRE(o.clip_idx == 0 || !r.masked, "same_overlap_noisy: the saved noisy tails belong to a different batch / overlap shape");
            // (the pair grows together; its shape is recorded once both exist)
            size_t got = 0;
            tails_blc = 0; tails_levels = 0;
            if (int e = grow_device_buffer(tails, got, r.blc * o.respacing, st)) return e;
            if (int e = grow_device_buffer(tail_tmp, got, r.blc, st)) return e;
            DSH_HIP_CHECK(hipMemsetAsync(tails, 0, r.blc * o.respacing * sizeof(float), st));
            tails_blc = r.blc; tails_levels = o.respacing;
        }
    }
    r.tail_gt = r.son && r.masked && o.clip_idx > 0;
    return 0;
}

// The chains the regime names.  More than one: every sub-batch runs the WHOLE loop on its own stream, forked from the context stream here and
// joined into it in finish(); else the whole batch on the context stream.
int Sampler::make_chains(Run& r) {
    ChainBufs& b = bufs[0];
    r.lag = (int)switch_int(SW_DUAL_LAG);
    const int ns = r.want.chains;
    if (ns <= 1) {
        r.chains.push_back(Chain{nullptr, st, 0, r.B, 0, r.n, r.w_lo, r.w_hi, b.nz1, b.nz_eta, b.t, b.c1, b.c2, b.lvl, &b});
        return 0;
    }
    for (int i = 0; i < ns; ++i) {
        Chain c{nullptr, nullptr, 0, 0, 0, 0, r.w_lo, r.w_hi, b.nz1, b.nz_eta, nullptr, nullptr, nullptr, b.lvl + i, &b};
        if (int e = r.den->sub_get(i, &c.inst, &c.s, &c.b0, &c.nb)) return e;
        c.off = (size_t)c.b0 * r.row_n; c.cnt = (size_t)c.nb * r.row_n;
        c.t = b.t + c.b0; c.c1 = b.c1 + c.b0; c.c2 = b.c2 + c.b0;
        r.chains.push_back(c);
    }
    if (!ev_fork) DSH_HIP_CHECK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    while (ev_sub.size() < 2 * r.chains.size()) { hipEvent_t e; DSH_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); ev_sub.push_back(e); }
    DSH_HIP_CHECK(hipEventRecord(ev_fork, st));
    for (size_t i = 1; i < r.chains.size(); ++i) DSH_HIP_CHECK(hipStreamWaitEvent(r.chains[i].s, ev_fork, 0));
    return 0;
}

// What the regime of a run depends on (loop_regime.h), and the schedule's first-use order beside it.  The only place of the sampling path
// that reads the regime switches: DSH_GRAPH_ROWS and the sampler's DSH_PIPE_ROWS as the process latched them, the others afresh.
LoopFacts Sampler::loop_facts(Run& r, const RunSpec& s) const {
    const SamplerOpts& o = r.o;
    LoopFacts f;
    f.kind = o.kind;
    f.batch = r.B; f.frames = r.den->frames(); f.channels = channels; f.gesture_cols = r.gcols; f.modality = r.mod;
    if (o.kind == 0) {
        std::vector<int> cnt(o.respacing, 0);
        for (const SamplerStep& sp : r.steps) if (sp.kind != STEP_UNDO) { ++f.evals; if (cnt[sp.level]++ == 0) { ++f.distinct; r.order.push_back(sp.level); } }
    }
    f.trace = r.trace != nullptr; f.same_overlap_noisy = o.same_overlap_noisy != 0; f.sync = !s.sync_left.empty(); f.profiling = prof && prof->on;
    f.cur_split = r.den->sub_count();
    f.graph_rows = (size_t)switch_int(SW_GRAPH_ROWS); f.no_graph = switch_present(SW_NO_GRAPH);
    f.level_cache = switch_int(SW_LEVEL_CACHE); f.level_prefetch = switch_int(SW_LEVEL_PREFETCH); f.pipe = switch_int(SW_PIPE);
    f.pipe_rows_context = r.den->unsplit_rows(); f.pipe_rows_sampler = pipe_rows();
    return f;
}

// Exactly what the regime names, asked of the denoiser in this order: graphs of the previous run dropped, the prefetch run begun (one level
// is queued now, the others one evaluation ahead of their first use: the host never runs far in front of the main chain, and the main chain
// never waits for the host to finish queueing 25 levels) or the cache slots prepared, the gesture-side twin started.  The fallbacks are for
// what can fail only at run time — an allocation, the slot cap of level_cache_prepare, a failed clone: prefetch -> inline cache if
// inline_ok -> none; pipeline -> one chain.
int Sampler::setup(Run& r) {
    const SamplerOpts& o = r.o;
    const LoopRegime& p = r.want;
    drop_graph();
    r.cache = p.cache;
    if (r.cache == CACHE_PREFETCH) {
        r.tv.resize(o.respacing);
        for (int k = 0; k < o.respacing; ++k) r.tv[k] = (int64_t)tb.tmap[k];
        if (r.den->level_prefetch(r.tv.data(), o.respacing, r.order.data(), 1, 1) == 0) r.pf_next = 1;
        else r.cache = p.inline_ok ? CACHE_INLINE : CACHE_NONE;
    }
    if (r.cache == CACHE_INLINE && r.den->level_cache_prepare(o.respacing) != 0) r.cache = CACHE_NONE;
    for (const Chain& c : r.chains) if (r.cache == CACHE_SUBS && c.inst->level_cache_prepare(o.respacing) != 0) r.cache = CACHE_NONE;
    if (r.cache != CACHE_NONE) r.level_seen.assign(o.respacing, 0);
    // (a DDIM twin restores its head from the slots of the prefetch run)
    ChainBufs& g = bufs[1];
    r.G = Chain{nullptr, nullptr, 0, r.B, 0, r.n, 0, r.gcols, g.nz1, g.nz_eta, g.t, g.c1, g.c2, g.lvl, &g};
    // (the gesture chain's scratch: ensure() sized it, the regime's own bound on n restates that size)
    const bool scratch_ok = g.nz1 && r.n <= cap_n2;
    if (p.pipe && scratch_ok && (o.kind == 1 || r.cache == CACHE_PREFETCH) && r.den->pipe_begin(&r.G.inst, &r.G.s) == 0) {
        r.piped = true;
        r.E = r.chains[0]; r.E.c_lo = r.gcols; r.E.c_hi = channels;
        for (hipEvent_t* e : {&ev_pE, &ev_pC, &ev_pG}) if (!*e) DSH_HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    return 0;
}

// the values of draw `idx` for one chain (device pointer; scratch = a full-size buffer the chain owns its element range of)
int Sampler::noise_for(const Run& r, int64_t idx, const Chain& c, float* scratch, const float** out) {
    const SamplerOpts& o = r.o;
    if (o.noise_mode == 0) { *out = r.noise_stack + (size_t)idx * r.n + c.off; return 0; }
    // (ragged: every row advances by its own size per draw, so a clip draws the same noise padded as sampled alone)
    if (r.per_row) { if (int e = launch_philox_randn_rows(scratch + c.off, c.nb, r.row_n, o.seed, (uint64_t)idx * r.quads, row_keys + c.b0, c.s,
                                                          r.len_d ? r.len_d + c.b0 : nullptr, (uint64_t)idx, channels,
                                                          r.seeds_d ? r.seeds_d + c.b0 : nullptr)) return e; }
    else if (int e = launch_philox_randn(scratch + c.off, c.cnt, o.seed, (uint64_t)idx * r.quads + c.off / 4, c.s)) return e;
    *out = scratch + c.off;
    return 0;
}

Sampler::StepConsts Sampler::step_consts(Run& r, const SamplerStep& sp) {
    const int k = sp.level;
    StepConsts sc{};
    sc.kind = sp.kind; sc.k = k; sc.eval_idx = -1; sc.idx = sc.idx2 = -1;
    if (sp.kind == STEP_UNDO) {
        const float beta = (float)tb.betas[k];
        sc.undo_a = sqrtf(1.0f - beta); sc.undo_b = sqrtf(beta);
        sc.idx = r.next_draw();
        return sc;
    }
    sc.eval_idx = r.n_eval++;
    sc.t = (int64_t)tb.tmap[k]; sc.c1 = (float)tb.c1[k]; sc.c2 = (float)tb.c2[k];
    if (sp.kind == STEP_REVERSE) {
        // ddim_reverse_sample (:1092-1102): x0 and eps as in the forward step, then x <- sqrt(ab_next) x0 + sqrt(1 - ab_next) eps — the
        // forward update with ab_next in the place of ab_prev, and no draw; sqrt taken in fp32 on the gathered fp32 value like the reference's th.sqrt
        const float abn = (float)tb.ac_next[k];
        sc.sqrt_ab_prev = sqrtf(abn);
        sc.sqrt_1m_ab_prev = sc.coef_eps = sqrtf(1.0f - abn);
        return sc;
    }
    sc.idx = r.next_draw();                                         // DDIM: randn_like of the step, times sigma (= 0 at eta = 0: drawn index, unused values)
    // (fp32 like the reference's gathered tensors: (1 - alpha_bar).sqrt() and p_mean_variance's "variance", gaussian_diffusion.py:670-673, :576)
    sc.sqrt_1m_ab = sqrtf(1.0f - (float)tb.ac[k]); sc.post_var = (float)tb.post_var[k];
    if (sp.kind == STEP_DDPM) {
        sc.coef1 = (float)tb.coef1[k]; sc.coef2 = (float)tb.coef2[k];
        sc.sigma = k == 0 ? 0.0f : expf(0.5f * (float)tb.post_logvar[k]);
        return sc;
    }
    // sigma = eta sqrt((1 - abar_prev) / (1 - abar)) sqrt(1 - abar / abar_prev), fp32 like the reference's tensors
    const float ab = (float)tb.ac[k], abp = (float)tb.ac_prev[k];
    sc.sqrt_ab_prev = sqrtf(abp);
    sc.sqrt_1m_ab_prev = sqrtf(1.0f - abp);
    sc.sigma = 0.f; sc.coef_eps = sqrtf(1.0f - abp);
    if (r.o.eta != 0.f) {
        sc.sigma = (r.o.eta * sqrtf((1.0f - abp) / (1.0f - ab))) * sqrtf(1.0f - ab / abp);
        sc.coef_eps = sqrtf((1.0f - abp) - sc.sigma * sc.sigma);
        if (k == 0) sc.sigma = 0.f;                                 // nonzero_mask: no noise at (spaced) t == 0; the mean keeps coef_eps
    }
    if (r.masked && !r.tail_gt) sc.idx2 = r.next_draw();            // N(0,1) of the noised gt (RePaint blend)
    if (r.dpm && k != 0 && r.last_ddim_level == k + 1) {
        double A, Bc, G;
        solver_coeffs(tb, k, A, Bc, G);
        sc.second = true; sc.sA = (float)A; sc.sBc = (float)Bc; sc.sG = (float)G;
    }
    return sc;
}

// the evaluation of a step, on every chain of the run (pipelined: the expression encoder's; gesture_follow() queues the twin's)
int Sampler::evaluate(Run& r, const StepConsts& sc) {
    const int k = sc.k;
    const LoopRegime& p = r.want; const std::vector<int>& order = r.order;
    const bool seen = r.cache != CACHE_NONE && r.level_seen[k];
    const int mode = r.cache == CACHE_NONE ? EVAL_PLAIN : (r.cache == CACHE_PREFETCH || seen) ? EVAL_RESTORE : EVAL_SAVE;
    // (pipelined: E_k overwrites the expression estimate the twin copied behind E_{k-1})
    if (r.piped && sc.eval_idx > 0) DSH_HIP_CHECK(hipStreamWaitEvent(st, ev_pC, 0));
    const bool first_eval = sc.eval_idx == 0;
    for (size_t i = 0; i < r.chains.size(); ++i) {
        const Chain& c = r.chains[i];
        if (int e = launch_fill_step(c.t, c.c1, c.c2, c.lvl, sc.t, sc.c1, sc.c2, (int64_t)k, c.nb, c.s)) return e;
        if (r.cache == CACHE_PREFETCH && !seen) {
            // first use: this level was queued one evaluation ago (or in setup()); queue the next new one now
            size_t pos = 0;
            while (pos < order.size() && order[pos] != k) ++pos;
            const size_t want = std::min(order.size(), pos + 2);
            if (want > r.pf_next) {
                if (int e = r.den->level_prefetch(r.tv.data(), r.o.respacing, order.data() + r.pf_next, (int)(want - r.pf_next), 0)) return e;
                r.pf_next = want;
            }
            if (int e = r.den->level_wait(k)) return e;
        }
        if (p.split()) {
            // every sub-batch on its own stream; at the very first evaluation sub-batch i + 1 starts a few launches behind
            // sub-batch i (so that the kernel sequences are out of phase from the start); afterwards the streams run free
            if (first_eval && i > 0) DSH_HIP_CHECK(hipStreamWaitEvent(c.s, ev_sub[2 * (i - 1)], 0));
            c.inst->notify_after_launches((first_eval && i + 1 < r.chains.size()) ? ev_sub[2 * i] : nullptr, r.lag);
            c.inst->t_uniform = r.den->t_uniform;
        }
        if (int e = eval_step(r, c, sc.eval_idx, p.graph, mode)) return e;
        if (p.split()) c.inst->notify_after_launches(nullptr, 0);
    }
    if (r.cache != CACHE_NONE) r.level_seen[k] = 1;
    return 0;
}

// Pipelined loop, between the two chains' updates of a step: E_k has advanced the expression channels on the context stream; G_k on the
// twin's takes E_k's x0 estimate and evaluates the gesture encoder at the same level (DDIM: head restored from the timestep cache, once the
// prefetch run has filled the level; DDPM: computed).  The caller then advances the gesture channels.
int Sampler::gesture_follow(Run& r, const StepConsts& sc) {
    const Chain& G = r.G;
    const int twin_mode = r.o.kind == 0 ? EVAL_RESTORE : EVAL_PLAIN;
    DSH_HIP_CHECK(hipEventRecord(ev_pE, st));
    DSH_HIP_CHECK(hipStreamWaitEvent(G.s, ev_pE, 0));
    if (int e = r.den->import_expr_into_twin(G.s)) return e;
    DSH_HIP_CHECK(hipEventRecord(ev_pC, G.s));
    if (int e = launch_fill_step(G.t, G.c1, G.c2, G.lvl, sc.t, sc.c1, sc.c2, (int64_t)sc.k, G.nb, G.s)) return e;
    if (twin_mode == EVAL_RESTORE) { if (int e = r.den->level_wait_stream(sc.k, G.s)) return e; }
    return eval_step(r, G, sc.eval_idx, r.want.graph, twin_mode);
}

int Sampler::ddim_update(Run& r, const Chain& c, const StepConsts& sc) {
    const SamplerOpts& o = r.o; const int k = sc.k;
    DdimStepArgs a;
    a.c_lo = c.c_lo; a.c_hi = c.c_hi;
    // (SOLVER_DPM2M: a first-order step is this launch, and leaves its x0 in the history)
    a.x = r.x + c.off; a.eps = eps + c.off; a.x0_out = (r.dpm && sc.kind == STEP_DDIM) ? hist + c.off : nullptr; a.c1 = sc.c1; a.c2 = sc.c2;
    a.sqrt_ab_prev = sc.sqrt_ab_prev; a.sqrt_1m_ab_prev = sc.sqrt_1m_ab_prev;
    a.coef_eps = sc.coef_eps; a.sigma = sc.sigma; a.noise1 = nullptr;
    if (o.eta != 0.f && sc.kind == STEP_DDIM) {
        // (nz1 is the scratch of the RePaint draw below: a second buffer only exists for eta != 0)
        const float* z1 = nullptr;
        if (int e = noise_for(r, sc.idx, c, c.nz_eta, &z1)) return e;
        a.noise1 = z1;
    }
    a.mask = nullptr; a.gt = nullptr; a.noise2 = nullptr; a.blend = 0; a.clip = o.clip_denoised;
    a.overlap_len = o.overlap_len; a.frames = r.den->frames(); a.channels = channels; a.n = c.cnt;
    const size_t toff = (size_t)c.b0 * o.overlap_len * channels;
    a.tail_in = nullptr; a.tail_out = r.son ? tail_tmp + toff : nullptr;
    if (r.masked) {
        const float* z2 = nullptr;
        if (r.tail_gt) a.tail_in = tails + (size_t)k * r.blc + toff;
        else if (int e = noise_for(r, sc.idx2, c, c.nz1, &z2)) return e;
        a.mask = r.mask + c.off; a.gt = r.gt + c.off; a.noise2 = z2;
        a.blend = (a.sqrt_1m_ab_prev < 0.2f && o.add_blend) ? 1 : 0;
        a.tail_blend = (a.blend && r.tail_blend) ? 1 : 0;
    }
    // (a second-order step reads the history it rewrites; no eta draw and no saved noisy tails under that solver: check_run())
    a.second = sc.second ? 1 : 0; a.A = sc.sA; a.Bc = sc.sBc; a.G = sc.sG;
    GuideArgs ga;
    if (sc.kind == STEP_DDIM && guide_for(r, c, sc, ga)) { if (int e = launch_guided_ddim_step(a, ga, c.s)) return e; }
    else if (int e = launch_ddim_step(a, c.s)) return e;
    if (r.son) DSH_HIP_CHECK(hipMemcpyAsync(tails + (size_t)k * r.blc + toff, tail_tmp + toff, (size_t)c.nb * o.overlap_len * channels * sizeof(float),
                                           hipMemcpyDeviceToDevice, c.s));
    return 0;
}

int Sampler::ddpm_update(Run& r, const Chain& c, const StepConsts& sc) {
    const float* z;
    if (int e = noise_for(r, sc.idx, c, c.nz1, &z)) return e;
    DdpmStepArgs a;
    a.x = r.x + c.off; a.eps = eps + c.off; a.noise = z; a.x0_out = nullptr; a.c1 = sc.c1; a.c2 = sc.c2;
    a.coef1 = sc.coef1; a.coef2 = sc.coef2; a.sigma = sc.sigma;
    a.n = c.cnt; a.clip = r.o.clip_denoised; a.channels = channels; a.c_lo = c.c_lo; a.c_hi = c.c_hi;
    GuideArgs ga;
    if (guide_for(r, c, sc, ga)) return launch_guided_ddpm_step(a, r.den->frames(), ga, c.s);
    return launch_ddpm_step(a, c.s);
}

// The guidance of one chain's share of a denoise step: its element range of target / weight, its clips' lengths, the level's scale.
// false: the step is the unguided launch (no guidance in the run, or a zero scale at this level).
// (Ragged batch: the guided launches leave the padded frames >= lens[b] unwritten while the unguided ones update them, so with zeros in
//  level_scale a padded frame is advanced at some levels and not at others.  Nothing reads those frames — the evaluation takes the clip's own
//  length, finish() zeroes them in the result — and rows of `trace` hold unspecified values there either way.)
bool Sampler::guide_for(const Run& r, const Chain& c, const StepConsts& sc, GuideArgs& g) const {
    if (!r.guide) return false;
    const Guidance& gd = *r.guide;
    const float scale = gd.level_scale.empty() ? 1.0f : gd.level_scale[sc.k];
    if (scale == 0.0f) return false;
    g.target = gd.target ? gd.target + c.off : nullptr; g.weight = gd.weight ? gd.weight + c.off : nullptr;
    g.vel = gd.vel; g.acc = gd.acc;
    g.lens = r.len_d ? r.len_d + c.b0 : nullptr;
    g.scale = scale; g.space = gd.space; g.sqrt_1m_ab = sc.sqrt_1m_ab; g.post_var = sc.post_var;
    return true;
}

// one chain's share of a step: its columns of its rows, on its stream (every chain draws the same values: the noise depends on the position only)
int Sampler::update(Run& r, const Chain& c, const StepConsts& sc) {
    if (sc.kind == STEP_DDIM || sc.kind == STEP_REVERSE) return ddim_update(r, c, sc);      // (reverse: check_run() admits no mask, eta, tails)
    if (sc.kind == STEP_DDPM) return ddpm_update(r, c, sc);
    const float* z;
    if (int e = noise_for(r, sc.idx, c, c.nz1, &z)) return e;
    return launch_undo_step(r.x + c.off, z, sc.undo_a, sc.undo_b, c.cnt, c.s, channels, c.c_lo, c.c_hi);
}

// Synchronised windows: behind its DDIM step the chain reconciles, on its own columns and stream, the frames neighbouring rows share.
int Sampler::window_sync(Run& r, const Chain& c) {
    return launch_window_sync(r.x + c.off, c.nb, r.den->frames(), channels, r.sync_d + c.b0, r.len_d ? r.len_d + c.b0 : nullptr, r.sync_len,
                              c.c_lo, c.c_hi, c.s);
}

// x at the schedule's first level.  init 0: draw 0 is x_T.  init 2: x holds x0; draw 0 — the draw x_T would have taken, through noise_for(), so
// row keys, row seeds and ragged lengths address it alike — is the q_sample noise, and every chain noises its rows and columns in place
// (coefficients: fp64 sqrt of the table rounded to fp32, like the reference's sqrt_alphas_cumprod tables; they travel in the chain's c1 / c2
// rows, which the first evaluation refills behind this launch on the same stream).
int Sampler::init_x(Run& r) {
    if (r.init == 1) return 0;
    const int64_t idx = r.next_draw();
    for (const Chain& c : r.chains) {
        const float* z;
        if (int e = noise_for(r, idx, c, r.init == 2 ? c.nz1 : r.x, &z)) return e;
        if (r.init == 0) {
            if (z != r.x + c.off) DSH_HIP_CHECK(hipMemcpyAsync(r.x + c.off, z, c.cnt * sizeof(float), hipMemcpyDeviceToDevice, c.s));
            continue;
        }
        const int k = r.steps.front().level;
        if (int e = launch_fill_step(c.t, c.c1, c.c2, c.lvl, (int64_t)tb.tmap[k], (float)sqrt(tb.ac[k]), (float)sqrt(1.0 - tb.ac[k]), (int64_t)k, c.nb, c.s)) return e;
        QSampleArgs a{};
        a.out = r.x + c.off; a.x0 = r.x + c.off; a.noise = z; a.a = c.c1; a.s = c.c2;
        a.n = c.cnt; a.frames = r.den->frames(); a.channels = channels; a.c_lo = c.c_lo; a.c_hi = c.c_hi; a.fixed_from = -1;
        if (int e = launch_q_sample(a, c.s)) return e;
    }
    return 0;
}

// Everything between the fork of make_chains() and the joins of finish(): any error leaves through `return`, and run() passes the result
// to finish() unconditionally.
int Sampler::loop(Run& r) {
    if (int e = init_x(r)) return e;
    if (int e = setup(r)) return e;
    for (const SamplerStep& sp : r.steps) {
        const StepConsts sc = step_consts(r, sp);
        if (sp.kind != STEP_UNDO) { if (int e = evaluate(r, sc)) return e; }
        if (r.piped) {
            // each chain advances its own channels on its own stream, the gesture chain behind the expression chain's evaluation of the step
            const bool sync = r.sync_d && sp.kind == STEP_DDIM;
            if (int e = update(r, r.E, sc)) return e;
            if (sync) { if (int e = window_sync(r, r.E)) return e; }
            if (sp.kind != STEP_UNDO) { if (int e = gesture_follow(r, sc)) return e; }
            if (int e = update(r, r.G, sc)) return e;
            if (sync) { if (int e = window_sync(r, r.G)) return e; }
        } else {
            for (const Chain& c : r.chains) {
                if (int e = update(r, c, sc)) return e;
                if (r.sync_d && sp.kind == STEP_DDIM) { if (int e = window_sync(r, c)) return e; }
            }
        }
        if (r.trace)
            for (const Chain& c : r.chains)
                DSH_HIP_CHECK(hipMemcpyAsync(r.trace + (size_t)r.step_idx * r.n + c.off, r.x + c.off, c.cnt * sizeof(float), hipMemcpyDeviceToDevice, c.s));
        r.last_ddim_level = sp.kind == STEP_DDIM ? sp.level : -1;
        ++r.step_idx;
    }
    return 0;
}

// the joins (on every exit path of loop(): the chains write x, trace and the noisy tails the caller may free) and what follows them
int Sampler::finish(Run& r, int rc) {
    DenoiserContext* den = r.den; const int B = r.B;
    note_launch_value(LC_SAMPLE_STREAMS, (long long)r.chains.size());
    note_launch_value(LC_SAMPLE_GRAPH, replayed() ? 1 : 0);
    note_launch_value(LC_SAMPLE_PIPE, r.piped ? 1 : 0);
    if (r.piped) {
        // both instances go back to whole evaluations (host state: before anything that can fail); the gesture chain joins the context stream
        (void)den->pipe_end();
        DSH_HIP_CHECK(hipEventRecord(ev_pG, r.G.s));
        DSH_HIP_CHECK(hipStreamWaitEvent(st, ev_pG, 0));
    }
    for (size_t i = 1; i < r.chains.size(); ++i) {
        DSH_HIP_CHECK(hipEventRecord(ev_sub[2 * i + 1], r.chains[i].s));
        DSH_HIP_CHECK(hipStreamWaitEvent(st, ev_sub[2 * i + 1], 0));
    }
    if (replayed()) { DSH_HIP_CHECK(hipStreamSynchronize(st)); drop_graph(); }
    // one modality alone: the inactive columns of the result are defined — 0, or the given track bit for bit — whatever x held there (one launch
    // behind the join, like the ragged zeroing that follows it)
    if (rc == 0 && r.mod == 1) { if (int e = launch_fill_cols(r.x, channels, (size_t)B * den->frames(), 0, r.gcols, nullptr, 0, st)) return e; }
    if (rc == 0 && r.mod == 2) {
        const float* track = den->modality_track();
        DSH_REQUIRE(track != nullptr, "gesture modality without its expression track");
        if (int e = launch_fill_cols(r.x, channels, (size_t)B * den->frames(), r.gcols, channels, track, channels - r.gcols, st)) return e;
    }
    // ragged batch: the loop ran on the padded rows; its result is defined as exactly 0 beyond every clip's length (one launch behind the join,
    // whatever regime the loop ran in; rows of `trace` keep the padded frames' values)
    if (rc == 0 && r.len_d) return launch_zero_padded_frames(r.x, r.len_d, B, den->frames(), channels, st);
    return rc;
}

int Sampler::run(DenoiserContext* den, const RunSpec& s) {
    DSH_REQUIRE(den && den->batch() > 0, "set_condition() must precede sample()");
    const SamplerOpts& o = s.o;
    const bool reverse = s.invert_to > 0;
    // every refusal, and the schedule, before anything changes in the context or on the device
    const RunShape shape{den->batch(), den->frames(), channels, den->gesture_channels(), den->modality(), den->lengths_host()};
    std::string err;
    Run r{den, o, s.x, reverse ? 1 : s.init, s.gt, s.mask, s.masked, s.noise_stack, s.trace, s.tail_blend};
    if (check_run(s, &shape, err) || plan_steps(s, r.steps, err)) { set_last_error(err); return -1; }
    DSH_REQUIRE(o.noise_mode != 0 || reverse || (s.noise_stack != nullptr && s.n_draws >= count_draws(s, r.steps)), "noise stack shorter than the loop's draw count");
    const int B = r.B = shape.batch;
    // One modality alone (denoiser.h, set_modality): the loop advances the active encoder's column window [w_lo, w_hi) only — every step launch
    // of every regime takes it — and its result holds 0 (expression mode) or the given track (gesture mode) in the other columns.  Noise
    // addressing stays that of the full-width row, so an active column receives the value it receives in the joint run.
    const int mod = r.mod = shape.modality, gcols = r.gcols = shape.gesture_cols;
    r.w_lo = mod == 1 ? gcols : 0; r.w_hi = mod == 0 ? 0 : (mod == 1 ? channels : gcols);      // (0, 0: all columns)
    r.guide = s.guide.on ? &s.guide : nullptr;
    r.len_d = den->lengths_dev();           // ragged batch (set_condition_ragged): per-clip frame counts of the padded batch, owned by the context
    // the regime, decided once, before anything changes in the context or on the device
    r.want = loop_regime(loop_facts(r, s));
    // loop_begin() marks the batch as deliberately unsplit; the mark is taken back on EVERY way out of this function (an argument error or a
    // failed launch below must not leave the context answering later evaluations as if a loop were still running)
    struct LoopScope { DenoiserContext* d; ~LoopScope() { (void)d->loop_end(); } } loop_scope{den};
    if (int e = den->loop_begin(r.want.unsplit)) return e;  // (may re-condition a mid-size batch as one batch: the two encoder chains replace the sub-batch streams)
    den->t_uniform = emb_dedup_enabled();   // every evaluation of a sampling loop runs the whole batch at ONE timestep (launch_fill_step)
    r.n = (size_t)B * den->frames() * channels; r.row_n = r.n / B;
    if (int e = prepare(r, s)) return e;
    if (int e = make_chains(r)) return e;
    // from the fork to the joins: loop() reports an error by returning, finish() joins the chains into the context stream whatever it returned
    const int rc = loop(r);
    return finish(r, rc);
}

}  // namespace dsh
