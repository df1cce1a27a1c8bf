// extern "C" surface of libdiffsheg_hip.so — see include/diffsheg_hip.h for the contract.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "../../include/diffsheg_hip.h"
#include "denoiser.h"
#include "audio_front.h"
#include "fgd.h"
#include "hubert.h"
#include "losses.h"
#include "sampler.h"

namespace dsh {
static thread_local std::string g_last_error;
void set_last_error(const std::string& msg) { g_last_error = msg; }
const char* last_error_cstr() { return g_last_error.c_str(); }
}  // namespace dsh

struct dsh_ctx {
    dsh::ModelConfig cfg;
    hipStream_t stream = nullptr;
    std::unique_ptr<dsh::DenoiserContext> den;
    std::unique_ptr<dsh::Sampler> sampler;
    dsh::RunSpec sticky;                               // what the dsh_sample_set_* setters hold for dsh_sample / dsh_invert (dsh_sample_run reads none of it)
    std::map<std::string, dsh::HostTensor> staged;
    dsh::Profiler prof;
    bool finalized = false;
    bool owns_stream = false;
    // guidance scales (dsh_set_guidance_scale): device buffer read by the mix kernels, n values (0 = the config's cond_scale, held as one);
    // the doubling decision is kept on the host
    float* gs_dev = nullptr;
    int gs_cap = 0, gs_n = 0;
    bool gs_dbl = false;
    // guidance schedule (dsh_set_guidance_schedule): [2 diffusion_steps gains | 2 phi] at one address for the life of the context, written in
    // stream order; sched_on: a schedule is set
    float* sched_dev = nullptr;
    bool sched_on = false;
    ~dsh_ctx() {
        den.reset();                                   // (the instances hold gs_dev and sched_dev)
        if (gs_dev) (void)hipFree(gs_dev);
        if (sched_dev) (void)hipFree(sched_dev);
    }
};

// n scales (n = 0: the config's cond_scale) -> the context's device buffer, in stream order, and the denoiser's doubling decision
static int set_guidance(dsh_ctx* ctx, const float* scales, int n) {
    DSH_REQUIRE(n >= 0 && (n == 0 || scales), "dsh_set_guidance_scale: null scale array");
    const std::vector<float> v = n ? std::vector<float>(scales, scales + n) : std::vector<float>{ctx->cfg.cond_scale};
    bool any = false;
    for (float x : v) {
        DSH_REQUIRE(std::isfinite(x), "dsh_set_guidance_scale: scales must be finite");
        any = any || x != 1.0f;
    }
    DSH_REQUIRE(!(any && n > 0 && !ctx->cfg.classifier_free), "dsh_set_guidance_scale: the weights are not classifier-free (no null_cond_emb): the scale must be 1");
    const int m = (int)v.size();
    if (m > ctx->gs_cap) {
        // (one allocation covers every batch up to 1024 clips: the address stays fixed for the life of the context in practice)
        const int cap = std::max(m, 1024);
        DSH_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        DSH_HIP_CHECK(hipDeviceSynchronize());         // (sub-batch / twin streams of an earlier run may still read the old buffer)
        float* p = nullptr;
        DSH_HIP_CHECK(hipMalloc((void**)&p, (size_t)cap * sizeof(float)));
        if (ctx->gs_dev) (void)hipFree(ctx->gs_dev);
        ctx->gs_dev = p; ctx->gs_cap = cap;
    }
    // (in stream order: evaluations enqueued earlier on the context stream still read the old values; no host sync)
    if (int e = dsh::launch_store_values_f32(ctx->gs_dev, v.data(), m, ctx->stream)) return e;
    const bool dbl = ctx->cfg.classifier_free && any;
    if (int e = ctx->den->set_guidance(ctx->gs_dev, m > 1 ? 1 : 0, dbl)) return e;
    ctx->gs_n = n; ctx->gs_dbl = dbl;
    return 0;
}

// per-clip scales must match the batch being evaluated / sampled
static int check_guidance(const dsh_ctx* ctx) {
    DSH_REQUIRE(ctx->gs_n <= 1 || ctx->gs_n == ctx->den->batch(), "dsh_set_guidance_scale: per-clip scales do not match the batch of set_condition()");
    return 0;
}

namespace dsh { std::atomic<long long> g_launch_counts[LC_COUNT]; }

#define API_BEGIN try {
#define API_END                                                                       \
    } catch (const std::exception& e) {                                               \
        dsh::set_last_error(std::string("exception: ") + e.what());                   \
        return -3;                                                                    \
    } catch (...) {                                                                   \
        dsh::set_last_error("unknown exception");                                     \
        return -3;                                                                    \
    }

extern "C" {

const char* dsh_last_error(void) { return dsh::last_error_cstr(); }
const char* dsh_version(void) { return "diffsheg_hip 0.1 (gfx950)"; }

int dsh_create(const dsh_model_config* c, void* hip_stream, dsh_ctx** out) {
    API_BEGIN
    DSH_REQUIRE(c && out, "null argument");
    DSH_REQUIRE(c->precision == DSH_PRECISION_FP32 || c->precision == DSH_PRECISION_BF16 || c->precision == DSH_PRECISION_BF16X3, "unknown precision");
    DSH_REQUIRE(c->dim_pose > 0 && c->expression_dim > 0 && c->style_dim > 0, "dims must be positive");
    int ndev = 0;
    DSH_HIP_CHECK(hipGetDeviceCount(&ndev));
    DSH_REQUIRE(ndev > 0, "no HIP device visible: this library has no CPU fallback");
    auto* ctx = new dsh_ctx();
    dsh::ModelConfig& m = ctx->cfg;
    m.dim_pose = c->dim_pose; m.expression_dim = c->expression_dim; m.style_dim = c->style_dim;
    m.classifier_free = c->classifier_free; m.cond_scale = c->cond_scale; m.latent_dim = c->latent_dim;
    m.ff_size = c->ff_size; m.num_layers = c->num_layers; m.num_heads = c->num_heads; m.audio_dim = c->audio_dim;
    m.aud_latent_dim = c->aud_latent_dim; m.hubert_dim = c->hubert_dim; m.hubert_enc_dim = c->hubert_enc_dim;
    m.precision = c->precision;
    m.single_transformer = c->single_transformer ? 1 : 0;
    DSH_REQUIRE(c->diffusion_steps >= 0, "diffusion_steps must not be negative (0: 1000)");
    m.diffusion_steps = c->diffusion_steps ? c->diffusion_steps : 1000;
    ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
    if (ctx->stream == nullptr) {
        // The legacy NULL stream cannot be graph-captured.  A BLOCKING stream keeps the implicit ordering with work
        // the caller enqueues on the NULL stream (PyTorch's default stream), so the boundary semantics do not change.
        DSH_HIP_CHECK(hipStreamCreateWithFlags(&ctx->stream, hipStreamDefault));
        ctx->owns_stream = true;
    }
    ctx->den.reset(dsh::make_denoiser(m, ctx->stream));
    ctx->sampler.reset(new dsh::Sampler(ctx->stream, m.channels()));
    ctx->prof.st = ctx->stream;
    ctx->den->set_profiler(&ctx->prof);
    ctx->sampler->prof = &ctx->prof;
    if (int e = set_guidance(ctx, nullptr, 0)) { dsh_destroy(ctx); return e; }
    *out = ctx;
    return 0;
    API_END
}

int dsh_destroy(dsh_ctx* ctx) {
    API_BEGIN
    if (!ctx) return 0;
    (void)hipStreamSynchronize(ctx->stream);
    hipStream_t s = ctx->owns_stream ? ctx->stream : nullptr;
    delete ctx;
    if (s) (void)hipStreamDestroy(s);
    return 0;
    API_END
}

int dsh_load_tensor(dsh_ctx* ctx, const char* name, const float* host_data, const int64_t* shape, int32_t ndim) {
    API_BEGIN
    DSH_REQUIRE(ctx && name && host_data && (shape || ndim == 0) && ndim >= 0, "null argument");
    DSH_REQUIRE(!ctx->finalized, "weights already finalized");
    dsh::HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { DSH_REQUIRE(shape[i] >= 0, "negative dim"); t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.data.assign(host_data, host_data + n);
    ctx->staged[name] = std::move(t);
    return 0;
    API_END
}

int dsh_finalize_weights(dsh_ctx* ctx) {
    API_BEGIN
    DSH_REQUIRE(ctx, "null context");
    DSH_REQUIRE(!ctx->finalized, "weights already finalized");
    if (int e = ctx->den->finalize(ctx->staged)) return e;
    ctx->staged.clear();
    ctx->finalized = true;
    return 0;
    API_END
}

int64_t dsh_weight_bytes(const dsh_ctx* ctx) { return ctx ? (int64_t)ctx->den->weight_bytes() : -1; }

int dsh_set_condition(dsh_ctx* ctx, int32_t batch, int32_t frames, const float* audio_emb, const float* person_id,
                      const float* hubert) {
    API_BEGIN
    DSH_REQUIRE(ctx, "null context");
    return ctx->den->set_condition(batch, frames, nullptr, audio_emb, person_id, hubert);
    API_END
}

int dsh_set_condition_ragged(dsh_ctx* ctx, int32_t batch, int32_t frames_pad, const int32_t* lengths_host, const float* audio_emb,
                             const float* person_id, const float* hubert) {
    API_BEGIN
    DSH_REQUIRE(ctx, "null context");
    DSH_REQUIRE(lengths_host, "set_condition_ragged: null lengths");
    return ctx->den->set_condition(batch, frames_pad, lengths_host, audio_emb, person_id, hubert);
    API_END
}

int dsh_eval(dsh_ctx* ctx, const float* x, const int64_t* t, const float* c1, const float* c2, float* eps) {
    API_BEGIN
    DSH_REQUIRE(ctx && t, "null context / timestep tensor");
    // the embedding Linears run on the distinct (timestep, speaker) rows when the whole batch is at one timestep (what every sampling loop
    // passes, gaussian_diffusion.py:1125): the caller's tensor is checked here, on the host (B x 8 bytes; dsh_sample never comes this way)
    {
        hipStream_t s = reinterpret_cast<hipStream_t>(ctx->stream);
        const int B = ctx->den->batch();
        DSH_REQUIRE(B > 0, "set_condition() must precede eval()");
        std::vector<int64_t> th((size_t)B);
        DSH_HIP_CHECK(hipMemcpyAsync(th.data(), t, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        DSH_HIP_CHECK(hipStreamSynchronize(s));
        bool uni = true;
        for (int b = 1; b < B; ++b) uni = uni && th[b] == th[0];
        ctx->den->t_uniform = uni && dsh::emb_dedup_enabled();
    }
    if (int e = check_guidance(ctx)) return e;
    if (int e = ctx->den->eval(x, t, c1, c2, eps)) return e;
    // one modality alone: the inactive encoder's columns of eps are 0 (it was not launched)
    if (const int mod = ctx->den->modality()) {
        const int g = ctx->den->gesture_channels(), Cc = ctx->cfg.channels();
        DSH_REQUIRE(g > 0 && g < Cc && eps, "a partial modality needs the UniDiffuser's two encoders");
        return dsh::launch_fill_cols(eps, Cc, (size_t)ctx->den->batch() * ctx->den->frames(), mod == 1 ? 0 : g, mod == 1 ? g : Cc, nullptr, 0, ctx->stream);
    }
    return 0;
    API_END
}

int dsh_set_modality(dsh_ctx* ctx, int32_t modality, const float* expression) {
    API_BEGIN
    DSH_REQUIRE(ctx, "null context");
    return ctx->den->set_modality(modality, expression);
    API_END
}

double dsh_eval_flops(const dsh_ctx* ctx) { return ctx ? ctx->den->issued_flops_per_eval() : -1.0; }

int dsh_profile_enable(dsh_ctx* ctx, int32_t enable) {
    API_BEGIN
    DSH_REQUIRE(ctx, "null context");
    DSH_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->prof.reset();
    ctx->prof.on = enable != 0;
    return 0;
    API_END
}

int dsh_profile_read(dsh_ctx* ctx, double* ms16, int64_t* launches16, double* flops16, double* bytes16) {
    API_BEGIN
    DSH_REQUIRE(ctx && ms16 && launches16 && flops16 && bytes16, "null argument");
    long long n[dsh::PROF_NCLASS];
    ctx->prof.read(ms16, n);
    for (int c = 0; c < dsh::PROF_NCLASS; ++c) { launches16[c] = n[c]; flops16[c] = ctx->prof.flops[c]; bytes16[c] = ctx->prof.bytes[c]; }
    return 0;
    API_END
}

int dsh_profile_class_info(const dsh_ctx* ctx, int32_t cls, const char** kernel, const char** role) {
    API_BEGIN
    DSH_REQUIRE(ctx && kernel && role && cls >= 0 && cls < dsh::PROF_NCLASS, "invalid argument");
    const dsh::ProfClassInfo& i = dsh::prof_class_info(cls, ctx->cfg.fp32_storage());
    *kernel = i.kernel; *role = i.role;
    return 0;
    API_END
}

int dsh_debug_copy(dsh_ctx* ctx, const char* what, float* out) {
    API_BEGIN
    DSH_REQUIRE(ctx && what, "null argument");
    return ctx->den->debug_copy(what, out);
    API_END
}

static dsh::SamplerOpts to_opts(const dsh_sampler_opts* o) {
    dsh::SamplerOpts s;
    s.kind = o->kind; s.diffusion_steps = o->diffusion_steps; s.respacing = o->respacing; s.jump_length = o->jump_length;
    s.jump_n_sample = o->jump_n_sample; s.overlap_len = o->overlap_len; s.add_blend = o->add_blend;
    s.no_resample = o->no_resample; s.no_repaint = o->no_repaint; s.clip_denoised = o->clip_denoised; s.noise_mode = o->noise_mode; s.seed = o->seed;
    s.same_overlap_noisy = o->same_overlap_noisy; s.clip_idx = o->clip_idx; s.eta = o->eta;
    return s;
}

// dsh_run_spec -> dsh::RunSpec: the caller's struct_size bytes, the rest 0 / null
static int to_spec(const dsh_sampler_opts* opts, const dsh_run_spec* c, dsh::RunSpec& s) {
    DSH_REQUIRE(opts && c, "null argument");
    DSH_REQUIRE(c->struct_size >= sizeof(uint32_t) && c->struct_size <= sizeof(dsh_run_spec), "dsh_run_spec: struct_size is larger than this library knows");
    dsh_run_spec f{};
    std::memcpy(&f, c, c->struct_size);
    DSH_REQUIRE(f.n_timesteps >= 0 && (f.n_timesteps == 0 || f.timesteps), "dsh_run_spec: null timestep list");
    DSH_REQUIRE(f.n_rows >= 0 && (f.n_rows == 0 || f.row_keys), "dsh_run_spec: null row key array");
    s.o = to_opts(opts); s.init = f.init; s.x = f.x; s.gt = f.gt; s.mask = f.mask; s.masked = f.masked != 0;
    s.noise_stack = f.noise_stack; s.n_draws = f.n_draws; s.trace = f.trace;
    s.start_level = f.start_level; s.invert_from = f.invert_from; s.invert_to = f.invert_to;
    s.kept.assign(f.timesteps, f.timesteps + f.n_timesteps);
    s.solver = f.solver; s.tail_blend = f.tail_blend != 0;
    s.row_keys.assign(f.row_keys, f.row_keys + f.n_rows);
    if (f.row_seeds) s.row_seeds.assign(f.row_seeds, f.row_seeds + f.n_rows);
    if (f.guidance) {
        DSH_REQUIRE(f.n_guide_scale >= 0 && (f.n_guide_scale == 0 || f.guide_scale), "dsh_run_spec: null guidance scale array");
        dsh::Guidance& g = s.guide;
        g.on = true; g.target = f.guide_target; g.weight = f.guide_weight; g.vel = f.guide_vel; g.acc = f.guide_acc; g.space = f.guide_space;
        g.batch = f.guide_batch; g.frames = f.guide_frames; g.channels = f.guide_channels;
        g.level_scale.assign(f.guide_scale, f.guide_scale + f.n_guide_scale);
    }
    DSH_REQUIRE(f.n_sync >= 0 && (f.n_sync == 0 || f.sync_left), "dsh_run_spec: null sync_left array");
    s.sync_left.assign(f.sync_left, f.sync_left + f.n_sync); s.sync_len = f.n_sync ? f.sync_len : 0;
    return 0;
}

int dsh_sample_run(dsh_ctx* ctx, const dsh_sampler_opts* opts, const dsh_run_spec* spec) {
    API_BEGIN
    DSH_REQUIRE(ctx, "null context");
    dsh::RunSpec s;
    if (int e = to_spec(opts, spec, s)) return e;
    if (int e = check_guidance(ctx)) return e;
    return ctx->sampler->run(ctx->den.get(), s);
    API_END
}

int dsh_sample_count(const dsh_sampler_opts* opts, const dsh_run_spec* spec, int64_t* n_draws, int64_t* n_steps) {
    API_BEGIN
    dsh::RunSpec s;
    if (int e = to_spec(opts, spec, s)) return e;
    return dsh::sampler_count(s, n_draws, n_steps);
    API_END
}

// ---- compatibility layer: the sticky values live in ctx->sticky, every entry builds a spec ------------------------------------------
// (the step count does not depend on the init mode: its entries only range-check theirs)
static int64_t count_of(bool draws, const dsh_sampler_opts* opts, int32_t masked, int32_t init, int32_t start_level, const int32_t* kept, int32_t n) {
    if (!opts || n < 0 || (n > 0 && !kept)) { dsh::set_last_error("null argument"); return -1; }
    if (init < 0 || init > 2) { dsh::set_last_error("unknown init mode"); return -1; }
    dsh::RunSpec s;
    s.o = to_opts(opts); s.masked = masked != 0; s.init = draws ? init : 1; s.start_level = start_level; s.kept.assign(kept, kept + n);
    int64_t out = 0;
    return dsh::sampler_count(s, draws ? &out : nullptr, draws ? nullptr : &out) ? -1 : out;
}
int64_t dsh_sample_num_draws(const dsh_sampler_opts* opts, int32_t masked, int32_t init_from_x) { return count_of(true, opts, masked, init_from_x != 0, 0, nullptr, 0); }
int64_t dsh_sample_num_steps(const dsh_sampler_opts* opts, int32_t masked) { return count_of(false, opts, masked, 0, 0, nullptr, 0); }
int64_t dsh_sample_num_draws_from(const dsh_sampler_opts* opts, int32_t masked, int32_t init, int32_t start_level) {
    return count_of(true, opts, masked, init, start_level, nullptr, 0);
}
int64_t dsh_sample_num_steps_from(const dsh_sampler_opts* opts, int32_t masked, int32_t init, int32_t start_level) {
    return count_of(false, opts, masked, init, start_level, nullptr, 0);
}
int64_t dsh_sample_num_draws_subset(const dsh_sampler_opts* opts, int32_t masked, int32_t init, int32_t start_level, const int32_t* kept, int32_t n) {
    return count_of(true, opts, masked, init, start_level, kept, n);
}
int64_t dsh_sample_num_steps_subset(const dsh_sampler_opts* opts, int32_t masked, int32_t init, int32_t start_level, const int32_t* kept, int32_t n) {
    return count_of(false, opts, masked, init, start_level, kept, n);
}

int dsh_sample_set_row_keys(dsh_ctx* ctx, const uint64_t* keys_host, int32_t n) {
    API_BEGIN
    DSH_REQUIRE(ctx, "null context");
    DSH_REQUIRE(n >= 0 && (n == 0 || keys_host), "set_row_keys: null key array");
    ctx->sticky.row_keys.assign(keys_host, keys_host + n);
    ctx->sticky.row_seeds.clear();               // (per-row seeds belong to the key set they were given for)
    return 0;
    API_END
}

int dsh_sample_set_row_seeds(dsh_ctx* ctx, const uint64_t* seeds_host, int32_t n) {
    API_BEGIN
    DSH_REQUIRE(ctx, "null context");
    DSH_REQUIRE(n >= 0 && (n == 0 || seeds_host), "set_row_seeds: null seed array");
    DSH_REQUIRE(n == 0 || (size_t)n == ctx->sticky.row_keys.size(), "set_row_seeds: needs the row keys set first, and one seed per row key");
    ctx->sticky.row_seeds.assign(seeds_host, seeds_host + n);
    return 0;
    API_END
}

int dsh_sample_set_tail_blend(dsh_ctx* ctx, int32_t on) {
    API_BEGIN
    DSH_REQUIRE(ctx, "null context");
    ctx->sticky.tail_blend = on != 0;
    return 0;
    API_END
}

int dsh_sample_set_start_level(dsh_ctx* ctx, int32_t level) {
    API_BEGIN
    DSH_REQUIRE(ctx, "null context");
    DSH_REQUIRE(level >= 0, "set_start_level: negative level");
    ctx->sticky.start_level = level;
    return 0;
    API_END
}

// (a malformed list is refused here and leaves the previous one in place)
int dsh_sample_set_timesteps(dsh_ctx* ctx, const int32_t* kept_host, int32_t n) {
    API_BEGIN
    DSH_REQUIRE(ctx, "null context");
    DSH_REQUIRE(n >= 0 && (n == 0 || kept_host), "set_timesteps: null timestep list");
    for (int i = 0; i < n; ++i) {
        DSH_REQUIRE(kept_host[i] >= 0, "set_timesteps: negative timestep");
        DSH_REQUIRE(i == 0 || kept_host[i] > kept_host[i - 1], "set_timesteps: timesteps must be strictly ascending");
    }
    ctx->sticky.kept.assign(kept_host, kept_host + n);
    return 0;
    API_END
}

int dsh_sample_set_solver(dsh_ctx* ctx, int32_t solver) {
    API_BEGIN
    DSH_REQUIRE(ctx, "null context");
    DSH_REQUIRE(solver == dsh::SOLVER_DDIM || solver == dsh::SOLVER_DPM2M, "set_solver: unknown solver (0 ddim, 1 dpm2m)");
    ctx->sticky.solver = solver;
    return 0;
    API_END
}

int dsh_set_guidance_scale(dsh_ctx* ctx, const float* scales_host, int32_t n) {
    API_BEGIN
    DSH_REQUIRE(ctx, "null context");
    return set_guidance(ctx, scales_host, n);
    API_END
}

int dsh_set_guidance_schedule(dsh_ctx* ctx, const float* gain_expression, const float* gain_gesture, int32_t n_steps, float rescale_expression,
                              float rescale_gesture) {
    API_BEGIN
    DSH_REQUIRE(ctx, "null context");
    if (n_steps == 0) {                                // cleared: every instance is back on the plain mix
        if (int e = ctx->den->set_guidance_schedule(nullptr, 0, false, false)) return e;
        ctx->sched_on = false;
        return 0;
    }
    const int n = ctx->cfg.diffusion_steps;
    DSH_REQUIRE(n_steps == n, "dsh_set_guidance_schedule: one gain per original timestep (n_steps must be the model's diffusion steps), or 0 to clear");
    DSH_REQUIRE(gain_expression && gain_gesture, "dsh_set_guidance_schedule: null gain row");
    DSH_REQUIRE(rescale_expression >= 0.0f && rescale_expression <= 1.0f && rescale_gesture >= 0.0f && rescale_gesture <= 1.0f,
                "dsh_set_guidance_schedule: the rescale factors must lie in [0, 1]");
    bool trivial = rescale_expression == 0.0f && rescale_gesture == 0.0f, same = rescale_expression == rescale_gesture;
    for (int i = 0; i < n; ++i) {
        DSH_REQUIRE(std::isfinite(gain_expression[i]) && std::isfinite(gain_gesture[i]), "dsh_set_guidance_schedule: gains must be finite");
        trivial = trivial && gain_expression[i] == 1.0f && gain_gesture[i] == 1.0f;
        same = same && gain_expression[i] == gain_gesture[i];
    }
    DSH_REQUIRE(trivial || ctx->cfg.classifier_free, "dsh_set_guidance_schedule: the weights are not classifier-free (no null_cond_emb): only gains of 1 without rescale are possible");
    DSH_REQUIRE(same || !ctx->cfg.single_transformer, "dsh_set_guidance_schedule: a single transformer has one encoder: the two rows and the two rescale factors must be equal");
    if (!ctx->sched_dev) DSH_HIP_CHECK(hipMalloc((void**)&ctx->sched_dev, ((size_t)2 * n + 2) * sizeof(float)));
    std::vector<float> v((size_t)2 * n + 2);
    std::copy(gain_expression, gain_expression + n, v.begin());
    std::copy(gain_gesture, gain_gesture + n, v.begin() + n);
    v[(size_t)2 * n] = rescale_expression; v[(size_t)2 * n + 1] = rescale_gesture;
    // (in stream order, like the scales: evaluations enqueued earlier still read the old table)
    if (int e = dsh::launch_store_values_f32(ctx->sched_dev, v.data(), (int)v.size(), ctx->stream)) return e;
    if (int e = ctx->den->set_guidance_schedule(ctx->sched_dev, n, rescale_expression > 0.0f, rescale_gesture > 0.0f)) return e;
    ctx->sched_on = true;
    return 0;
    API_END
}

int dsh_sample(dsh_ctx* ctx, const dsh_sampler_opts* opts, float* x, int32_t init_from_x, const float* gt,
               const uint8_t* mask, int32_t masked, const float* noise_stack, int64_t n_draws, float* trace) {
    API_BEGIN
    DSH_REQUIRE(ctx && opts, "null argument");
    if (int e = check_guidance(ctx)) return e;
    DSH_REQUIRE(init_from_x >= 0 && init_from_x <= 2, "init_from_x: 0 (x_T is drawn), 1 (x is given) or 2 (x holds x0)");
    dsh::RunSpec s = ctx->sticky;                 // the setters' values, completed by this call's arguments
    s.o = to_opts(opts); s.init = init_from_x; s.x = x; s.gt = gt; s.mask = mask; s.masked = masked != 0;
    s.noise_stack = noise_stack; s.n_draws = n_draws; s.trace = trace;
    return ctx->sampler->run(ctx->den.get(), s);
    API_END
}

int dsh_invert_from(dsh_ctx* ctx, const dsh_sampler_opts* opts, float* x, int32_t from_level, int32_t to_level, float* trace) {
    API_BEGIN
    DSH_REQUIRE(ctx && opts, "null argument");
    if (int e = check_guidance(ctx)) return e;
    DSH_REQUIRE(to_level >= 1, "invert: needs 0 <= from_level < to_level");
    dsh::RunSpec s = ctx->sticky;                 // (a sticky start level or tail blend is refused, as documented; solver and row keys are not read)
    s.o = to_opts(opts); s.x = x; s.trace = trace; s.invert_from = from_level; s.invert_to = to_level;
    return ctx->sampler->run(ctx->den.get(), s);
    API_END
}
int dsh_invert(dsh_ctx* ctx, const dsh_sampler_opts* opts, float* x, int32_t to_level, float* trace) {
    return dsh_invert_from(ctx, opts, x, 0, to_level, trace);
}

static int32_t copy_table(const dsh::DiffusionTables& tb, const char* name, double* out, int32_t cap) {
    const std::string n(name);
    const std::vector<double>* v = nullptr;
    if (n == "betas") v = &tb.betas;
    else if (n == "alphas_cumprod") v = &tb.ac;
    else if (n == "alphas_cumprod_prev") v = &tb.ac_prev;
    else if (n == "alphas_cumprod_next") v = &tb.ac_next;
    else if (n == "sqrt_recip_alphas_cumprod") v = &tb.c1;
    else if (n == "sqrt_recipm1_alphas_cumprod") v = &tb.c2;
    else if (n == "posterior_variance") v = &tb.post_var;
    else if (n == "posterior_log_variance_clipped") v = &tb.post_logvar;
    else if (n == "posterior_mean_coef1") v = &tb.coef1;
    else if (n == "posterior_mean_coef2") v = &tb.coef2;
    DSH_REQUIRE(v != nullptr, "unknown table name");
    DSH_REQUIRE((int32_t)v->size() <= cap, "output buffer too small");
    std::memcpy(out, v->data(), v->size() * sizeof(double));
    return (int32_t)v->size();
}

int32_t dsh_diffusion_table(int32_t diffusion_steps, int32_t respacing, const char* name, double* out, int32_t cap) {
    API_BEGIN
    DSH_REQUIRE(name && out, "null argument");
    dsh::DiffusionTables tb; std::string err;
    if (dsh::make_tables(diffusion_steps, respacing, tb, err)) { dsh::set_last_error(err); return -1; }
    return copy_table(tb, name, out, cap);
    API_END
}

int32_t dsh_diffusion_table_subset(int32_t diffusion_steps, const int32_t* kept, int32_t n, const char* name, double* out, int32_t cap) {
    API_BEGIN
    DSH_REQUIRE(name && out && kept && n > 0, "null argument / empty subset");
    dsh::DiffusionTables tb; std::string err;
    if (dsh::make_tables_kept(diffusion_steps, std::vector<int>(kept, kept + n), tb, err)) { dsh::set_last_error(err); return -1; }
    return copy_table(tb, name, out, cap);
    API_END
}

int dsh_solver_coeffs(int32_t diffusion_steps, const int32_t* kept, int32_t n, int32_t k, double* out3) {
    API_BEGIN
    DSH_REQUIRE(out3 && kept && n > 0, "null argument / empty subset");
    DSH_REQUIRE(k >= 0 && k < n, "solver_coeffs: level outside 0 .. n - 1");
    dsh::DiffusionTables tb; std::string err;
    if (dsh::make_tables_kept(diffusion_steps, std::vector<int>(kept, kept + n), tb, err)) { dsh::set_last_error(err); return -1; }
    dsh::solver_coeffs(tb, k, out3[0], out3[1], out3[2]);
    return 0;
    API_END
}

int32_t dsh_masked_start_level(int32_t diffusion_steps, const int32_t* kept, int32_t n) {
    API_BEGIN
    DSH_REQUIRE(n >= 0 && (n == 0 || kept), "null argument");
    std::string err;
    const int t = dsh::masked_start_level(diffusion_steps, std::vector<int>(kept, kept + n), err);
    if (t < 0) dsh::set_last_error(err);
    return t;
    API_END
}

int32_t dsh_timestep_map(int32_t diffusion_steps, int32_t respacing, int32_t* out, int32_t cap) {
    API_BEGIN
    DSH_REQUIRE(out, "null argument");
    dsh::DiffusionTables tb; std::string err;
    if (dsh::make_tables(diffusion_steps, respacing, tb, err)) { dsh::set_last_error(err); return -1; }
    DSH_REQUIRE((int32_t)tb.tmap.size() <= cap, "output buffer too small");
    for (size_t i = 0; i < tb.tmap.size(); ++i) out[i] = tb.tmap[i];
    return (int32_t)tb.tmap.size();
    API_END
}

int32_t dsh_jump_schedule(int32_t respacing, int32_t jump_length, int32_t jump_n_sample, int32_t* out, int32_t cap) {
    API_BEGIN
    DSH_REQUIRE(out && respacing > 0 && jump_length > 0 && jump_n_sample > 0, "invalid argument");
    const std::vector<int> ts = dsh::jump_schedule(respacing, jump_length, jump_n_sample);
    DSH_REQUIRE((int32_t)ts.size() <= cap, "output buffer too small");
    for (size_t i = 0; i < ts.size(); ++i) out[i] = ts[i];
    return (int32_t)ts.size();
    API_END
}

// ---- unit kernels ---------------------------------------------------------------------------
int dsh_op_gemm(void* hip_stream, int32_t dtype, const void* A, const void* W, const float* bias, const float* R,
                float* Cf, void* Ct, int32_t M, int32_t N, int32_t K, int32_t act) {
    API_BEGIN
    dsh::GemmArgs a;
    a.A = A; a.lda = K; a.W = W; a.ldw = K; a.bias = bias; a.R = R; a.ldr = N; a.res_mod = 0; a.Cf = Cf; a.ldcf = N;
    a.Ct = Ct; a.ldct = N; a.M = M; a.N = N; a.K = K; a.act = act; a.act_after_res = 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    if (dtype == 0) return dsh::launch_gemm_f32(a, s);
    if (dtype == 1) return dsh::launch_gemm_bf16(a, s);
    dsh::set_last_error("dsh_op_gemm: unknown dtype");
    return -1;
    API_END
}

int dsh_op_gemm_ex(void* hip_stream, int32_t dtype, const void* A, const void* W, const float* bias, const float* R, float* Cf, void* Ct,
                   int32_t M, int32_t N, int32_t K, int32_t act, int32_t lda, int32_t ldw, int32_t ldr, int32_t res_mod, int32_t ldcf,
                   int32_t ldct, int32_t act_after_res) {
    API_BEGIN
    dsh::GemmArgs a;
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.bias = bias; a.R = R; a.ldr = ldr; a.res_mod = res_mod; a.Cf = Cf; a.ldcf = ldcf;
    a.Ct = Ct; a.ldct = ldct; a.M = M; a.N = N; a.K = K; a.act = act; a.act_after_res = act_after_res; a.nt_n = a.nt_m = 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    if (dtype == 0) return dsh::launch_gemm_f32(a, s);
    if (dtype == 1) return dsh::launch_gemm_bf16(a, s);
    dsh::set_last_error("dsh_op_gemm_ex: unknown dtype");
    return -1;
    API_END
}

int32_t dsh_debug_last_tl_variant(void) { return dsh::g_tl_last_variant; }

int32_t dsh_debug_launch_counts(int64_t* out, int32_t cap, int32_t reset) {
    for (int i = 0; i < dsh::LC_COUNT; ++i) {
        const long long v = reset ? dsh::g_launch_counts[i].exchange(0, std::memory_order_relaxed) : dsh::g_launch_counts[i].load(std::memory_order_relaxed);
        if (out && i < cap) out[i] = (int64_t)v;
    }
    return dsh::LC_COUNT;
}

// dsh_loop_facts -> dsh::LoopFacts -> loop_regime() -> dsh_loop_regime: the caller's struct_size bytes of either struct, the rest 0
int dsh_debug_loop_regime(const dsh_loop_facts* facts, dsh_loop_regime* regime) {
    API_BEGIN
    DSH_REQUIRE(facts && regime, "null argument");
    DSH_REQUIRE(facts->struct_size >= sizeof(uint32_t) && facts->struct_size <= sizeof(dsh_loop_facts), "dsh_loop_facts: struct_size is larger than this library knows");
    DSH_REQUIRE(regime->struct_size >= sizeof(uint32_t) && regime->struct_size <= sizeof(dsh_loop_regime), "dsh_loop_regime: struct_size is larger than this library knows");
    dsh_loop_facts c{};
    std::memcpy(&c, facts, facts->struct_size);
    DSH_REQUIRE(c.batch > 0 && c.frames > 0 && c.channels > 0 && (c.kind == 0 || c.kind == 1), "dsh_loop_facts: empty batch or unknown loop kind");
    dsh::LoopFacts f;
    f.kind = c.kind; f.batch = c.batch; f.frames = c.frames; f.channels = c.channels; f.gesture_cols = c.gesture_cols; f.modality = c.modality;
    f.evals = c.evals; f.distinct = c.distinct_levels;
    f.trace = c.trace != 0; f.same_overlap_noisy = c.same_overlap_noisy != 0; f.sync = c.sync != 0; f.profiling = c.profiling != 0;
    f.cur_split = c.cur_split;
    f.graph_rows = (size_t)c.graph_rows; f.no_graph = c.no_graph != 0;
    f.level_cache = c.level_cache; f.level_prefetch = c.level_prefetch; f.pipe = c.pipe;
    f.pipe_rows_context = (size_t)c.pipe_rows_context; f.pipe_rows_sampler = (size_t)c.pipe_rows_sampler;
    const dsh::LoopRegime r = dsh::loop_regime(f);
    dsh_loop_regime o{};
    o.struct_size = regime->struct_size;
    o.unsplit = r.unsplit; o.chains = r.chains; o.forked_evals = r.forked_evals; o.graph = r.graph; o.cache = (int32_t)r.cache;
    o.inline_ok = r.inline_ok; o.pipe = r.pipe;
    std::memcpy(regime, &o, regime->struct_size);
    return 0;
    API_END
}

// ---- op-level entries: test / bench helpers over ROW-MAJOR operands. Each builds the kernels' operands in per-call scratch, caches nothing
// (a cache keyed on a pointer would alias when the caller's allocator reuses the address) and frees the scratch after a stream sync.
namespace {
struct OpScratch {
    std::vector<void*> p;
    ~OpScratch() { for (void* q : p) (void)hipFree(q); }
    int alloc(void** out, size_t bytes) { DSH_HIP_CHECK(hipMalloc(out, bytes)); p.push_back(*out); return 0; }
    int upload(void** out, const void* host, size_t bytes) {
        if (int e = alloc(out, bytes)) return e;
        DSH_HIP_CHECK(hipMemcpy(*out, host, bytes, hipMemcpyHostToDevice));
        return 0;
    }
    // zeroed 64-bit words for a bench hook of the token-per-lane kernels (block timeline: 4 per block, phase probe: 8 per block)
    int words(unsigned long long** out, size_t n, hipStream_t s) {
        if (int e = alloc(reinterpret_cast<void**>(out), n * 8)) return e;
        DSH_HIP_CHECK(hipMemsetAsync(*out, 0, n * 8, s));
        return 0;
    }
};
int fetch_f32(std::vector<float>& dst, const float* dev, size_t n) {
    dst.resize(n);
    DSH_HIP_CHECK(hipMemcpy(dst.data(), dev, n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
// a bf16 device tensor as fp32 on the host (exact): the form the production packers take their weights in
int fetch_bf16_as_f32(std::vector<float>& dst, const void* dev, size_t n) {
    std::vector<dsh::bf16> raw(n);
    DSH_HIP_CHECK(hipMemcpy(raw.data(), dev, n * 2, hipMemcpyDeviceToHost));
    dst.resize(n);
    for (size_t i = 0; i < n; ++i) dst[i] = dsh::bf16_to_f32(raw[i]);
    return 0;
}
int fetch_words(std::vector<unsigned long long>& dst, const unsigned long long* dev, size_t n, hipStream_t s) {
    dst.resize(n);
    DSH_HIP_CHECK(hipStreamSynchronize(s));
    DSH_HIP_CHECK(hipMemcpy(dst.data(), dev, n * 8, hipMemcpyDeviceToHost));
    return 0;
}
// DSH_TL_TRACE: one line per block — index, three 100 MHz time stamps, then the two halves of the fourth word; skip_idle leaves out
// the slots no block wrote (the Linear's upper bound on its grid)
int dump_tl_trace(const char* path, const unsigned long long* dev, size_t nblk, bool skip_idle, hipStream_t s) {
    std::vector<unsigned long long> ht;
    if (int e = fetch_words(ht, dev, nblk * 4, s)) return e;
    if (FILE* f = fopen(path, "w")) {
        for (size_t i = 0; i < nblk; ++i)
            if (!skip_idle || ht[4 * i]) fprintf(f, "%zu %llu %llu %llu %llu %llu\n", i, ht[4 * i], ht[4 * i + 1], ht[4 * i + 2], ht[4 * i + 3] & 0xffffffffull, ht[4 * i + 3] >> 32);
        fclose(f);
    }
    return 0;
}
// DSH_TL_PROBE: one line per block — index and the first `nwords` of its 8 probe words (Linear 7, fused FFN 8)
int dump_tl_probe(const char* path, const unsigned long long* dev, size_t npb, int nwords, hipStream_t s) {
    std::vector<unsigned long long> hp;
    if (int e = fetch_words(hp, dev, npb * 8, s)) return e;
    if (FILE* f = fopen(path, "w")) {
        for (size_t i = 0; i < npb; ++i) {
            fprintf(f, "%zu", i);
            for (int k = 0; k < nwords; ++k) fprintf(f, " %llu", hp[8 * i + k]);
            fprintf(f, "\n");
        }
        fclose(f);
    }
    return 0;
}
}  // namespace

int dsh_op_gemm_f32_pro(void* hip_stream, int32_t pro, const float* x0, int32_t ld0, int32_t w0, const float* x1, int32_t ld1, int32_t w1,
                        const float* x2, int32_t ld2, int32_t w2, const float* x3, int32_t ld3, int32_t w3, int32_t k_real, const float* W,
                        const float* bias, const float* fc, const float* film, int32_t film_ld, int32_t film_off, int32_t frames, int32_t nb,
                        const float* R, float* C, int32_t M, int32_t N, int32_t act, const float* stats, int32_t stat_groups, float* stats_out) {
    return dsh_op_gemm_f32_pro_ex(hip_stream, pro, x0, ld0, w0, x1, ld1, w1, x2, ld2, w2, x3, ld3, w3, k_real, W, bias, fc, film, film_ld, film_off, frames, nb,
                                  R, C, M, N, act, stats, stat_groups, stats_out, 0);
}

int dsh_op_split_pack_weight(void* hip_stream, const float* W, int32_t N, int32_t K, void* out) {
    API_BEGIN
    return dsh::launch_split_pack_weight(W, N, K, K, reinterpret_cast<uint32_t*>(out), reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_gemm_f32_pro_ex(void* hip_stream, int32_t pro, const float* x0, int32_t ld0, int32_t w0, const float* x1, int32_t ld1, int32_t w1,
                           const float* x2, int32_t ld2, int32_t w2, const float* x3, int32_t ld3, int32_t w3, int32_t k_real, const float* W,
                           const float* bias, const float* fc, const float* film, int32_t film_ld, int32_t film_off, int32_t frames, int32_t nb,
                           const float* R, float* C, int32_t M, int32_t N, int32_t act, const float* stats, int32_t stat_groups, float* stats_out,
                           int32_t mma) {
    API_BEGIN
    const bool packed = mma > 0 && (mma & 64) != 0;          // W is the packed operand already (dsh_op_split_pack_weight)
    if (mma > 0) mma &= ~64;
    DSH_REQUIRE(mma == 0 || ((mma & 15) == 1 && (mma >> 4) >= 0 && (mma >> 4) <= 2), "mma: 0 (exact fp32) or 1 (split bf16) + 16 x tile (0 .. 2) [+ 64: W packed]");
    DSH_REQUIRE(w0 > 0 && w0 % 32 == 0 && w1 % 32 == 0 && w2 % 32 == 0 && w3 % 32 == 0 && w1 >= 0 && w2 >= 0 && w3 >= 0, "segment widths must be multiples of 32");
    dsh::GemmProArgs a{};
    a.pro = pro;
    a.seg[0] = x0; a.seg[1] = w1 ? x1 : nullptr; a.seg[2] = w2 ? x2 : nullptr; a.seg[3] = w3 ? x3 : nullptr;
    a.seg_ld[0] = ld0; a.seg_ld[1] = ld1; a.seg_ld[2] = ld2; a.seg_ld[3] = ld3;
    a.seg_end[0] = w0 / 32; a.seg_end[1] = a.seg_end[0] + w1 / 32; a.seg_end[2] = a.seg_end[1] + w2 / 32; a.seg_end[3] = a.seg_end[2] + w3 / 32;
    a.K = 32 * a.seg_end[3]; a.k_real = k_real;
    a.W = W; a.ldw = a.K; a.bias = bias; a.fc = fc;
    a.film = film; a.film_ld = film_ld; a.film_off = film_off; a.frames = frames; a.bmod = nb;
    a.R = R; a.ldr = N; a.C = C; a.ldc = N; a.M = M; a.N = N; a.act = act; a.nt_n = a.nt_m = 0;
    a.stats = stats; a.stat_groups = stat_groups; a.stat_gs = stat_groups > 0 ? a.K / stat_groups : 0; a.stats_out = stats_out;
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    if (mma == 0) return dsh::launch_gemm_f32_pro(a, s);
    // split bf16: the weight is packed into per-call scratch (the denoiser packs once, at finalisation), released after a stream sync
    DSH_REQUIRE(W && M > 0 && N > 0 && a.K > 0, "gemm_f32_pro: W and positive sizes");
    a.mma = 1; a.tile = mma >> 4;
    if (packed) return dsh::launch_gemm_f32_pro(a, s);
    OpScratch scratch;
    void* wsp = nullptr;
    if (int e = scratch.alloc(&wsp, (size_t)N * a.K * 4)) return e;
    if (int e = dsh::launch_split_pack_weight(W, N, a.K, a.K, reinterpret_cast<uint32_t*>(wsp), s)) return e;
    a.W = reinterpret_cast<const float*>(wsp);
    const int rc = dsh::launch_gemm_f32_pro(a, s);
    DSH_HIP_CHECK(hipStreamSynchronize(s));
    return rc;
    API_END
}

int dsh_op_tl_linear(void* hip_stream, int32_t pro, const void* X, const void* W, const float* bias, const float* R,
                     float* Cf, void* Ct, int32_t M, int32_t N, int32_t act, const float* gamma, const float* beta,
                     const float* film, int32_t frames, int32_t nb, int32_t K) {
    API_BEGIN
    DSH_REQUIRE(X && W && M > 0 && N > 0 && N % 32 == 0 && (K == 512 || K == 1024), "invalid argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    // The weight rows are pi-permuted and the row tensors converted to / from the kernel's tiled layouts in the per-call scratch
    // (finalize() / the denoiser do this once, or never leave the tiled layout).
    // DSH_TL_RAW=1 (timing loops only): every operand is passed through untouched as if already permuted / tiled / folded.
    OpScratch scratch;
    const bool raw = dsh::switch_int(dsh::SW_TL_RAW) != 0;
    const bool gen2 = dsh::switch_int(dsh::SW_TL2) != 0;   // second-generation (LDS-DMA) kernels unless DSH_TL2=0
    const size_t Mp = (size_t)dsh::round_up(M, 256) + 256;
    const float *fold_c = nullptr, *fold_d = nullptr;
    dsh::TlArgs a;
    a.X = X; a.R = R; a.Cf = Cf; a.Ct = Ct; a.W = W; a.film = film; a.Rlo = nullptr; a.Clo = nullptr;
    void* tcat[4] = {nullptr, nullptr, nullptr, nullptr};
    bool hilo = false;
    void *trl = nullptr, *tcl = nullptr;
    DSH_REQUIRE(pro != 3 || (K == 1024 && frames > 896 - 1 && frames <= 1024), "tl_linear pro 3: K = 1024, frames = real concat width (896 .. 1024)");
    if (!raw) {
        void *wpack = nullptr, *tx = nullptr, *tr = nullptr, *tcf = nullptr, *tct = nullptr;
        {   // the PRODUCTION packer (tl_pack_linear, as finalize() runs it) on the caller's weight, bf16 -> fp32 being exact: the first generation
            // takes the pi-permuted rows, the LDS-DMA kernels the fragment-ordered copy with the LayerNorm of pro 1 / 3 folded into it
            const bool fold = gen2 && (pro == 1 || pro == 3);
            std::vector<float> hw, hbias, hg, hb, hc(N), hd(N);
            std::vector<uint16_t> perm((size_t)N * K), frag((size_t)N * K);
            DSH_HIP_CHECK(hipStreamSynchronize(s));
            if (int e = fetch_bf16_as_f32(hw, W, (size_t)N * K)) return e;
            if (fold) {
                if (int e = fetch_f32(hg, gamma, K)) return e;
                if (int e = fetch_f32(hb, beta, K)) return e;
                if (bias) { if (int e = fetch_f32(hbias, bias, N)) return e; }
            }
            dsh::tl_pack_linear(hw.data(), hbias.empty() ? nullptr : hbias.data(), N, K, K, fold ? hg.data() : nullptr, fold ? hb.data() : nullptr,
                                perm.data(), frag.data(), hc.data(), hd.data());
            if (int e = scratch.upload(&wpack, gen2 ? frag.data() : perm.data(), (size_t)N * K * 2)) return e;
            a.W = wpack;
            if (fold) {
                void *dc = nullptr, *dd = nullptr;
                if (int e = scratch.upload(&dc, hc.data(), N * 4)) return e;
                if (int e = scratch.upload(&dd, hd.data(), N * 4)) return e;
                fold_c = reinterpret_cast<const float*>(dc); fold_d = reinterpret_cast<const float*>(dd);
            }
        }
        if (pro == 3) {
            // concat prologue (feat_proj.0 over [h | audio_proj | hubert128 | expr], transformer.py:304-312): the caller's row-major
            // [M, 1024] row is cut into the four tiled tensors the kernel reads; LayerNorm over the first `frames` (= kreal) columns
            const dsh::bf16* xb = reinterpret_cast<const dsh::bf16*>(X);
            const int offs[4] = {0, 512, 768, 896}, wid[4] = {512, 256, 128, 128};
            for (int i = 0; i < 4; ++i) {
                if (int e = scratch.alloc(&tcat[i], Mp * wid[i] * 2)) return e;
                if (int e = dsh::launch_tile_rows_bf16<dsh::bf16>(xb + offs[i], K, M, wid[i], tcat[i], wid[i], s)) return e;
            }
            a.X = tcat[0];
        } else {
            if (int e = scratch.alloc(&tx, Mp * K * 2)) return e;
            if (int e = dsh::launch_tile_rows_bf16<dsh::bf16>(reinterpret_cast<const dsh::bf16*>(X), K, M, K, tx, K, s)) return e;
            a.X = tx;
        }
        // DSH_HILO=1 (tests of the hi / lo residual planes, tl_common.h): a residual-carrying call with both outputs runs the plane
        // instantiation — R is split into (hi, lo) planes, Cf comes back as hi + lo and Ct as the hi plane
        hilo = dsh::hilo_op() && R && Cf && Ct && act == 0 && ((pro == 2 && K == 512) || (pro == 0 && K == 1024));
        if (hilo) {
            if (int e = scratch.alloc(&tr, Mp * N * 2)) return e;
            if (int e = scratch.alloc(&trl, Mp * N * 2)) return e;
            if (int e = dsh::launch_tile_rows_hilo(R, N, M, N, tr, trl, N, s)) return e;
            if (int e = scratch.alloc(&tct, Mp * N * 2)) return e;
            if (int e = scratch.alloc(&tcl, Mp * N * 2)) return e;
            a.R = reinterpret_cast<const float*>(tr); a.Rlo = trl; a.Cf = nullptr; a.Ct = tct; a.Clo = tcl;
        } else {
        if (R) { if (int e = scratch.alloc(&tr, Mp * N * 4)) return e;
                 if (int e = dsh::launch_tile_rows_f32(R, N, M, reinterpret_cast<float*>(tr), N, s)) return e;
                 a.R = reinterpret_cast<const float*>(tr); }
        if (Cf) { if (int e = scratch.alloc(&tcf, Mp * N * 4)) return e; a.Cf = reinterpret_cast<float*>(tcf); }
        if (Ct) { if (int e = scratch.alloc(&tct, Mp * N * 2)) return e; a.Ct = tct; }
        }
    }
    a.ldx = K; a.K = K; a.bias = bias; a.ldr = N; a.ldcf = N; a.cf_rowmajor = 0; a.ldct = N; a.half_row0 = 0x7fffffff;
    a.M = M; a.N = N; a.act = act; a.gamma = gamma; a.beta = beta; a.film_ld = 2 * K; a.film_off = 0;
    a.frames = frames > 0 ? frames : 1; a.bmod = nb > 0 ? nb : 1; a.row_const = nullptr; a.n_const_rows = 0;
    a.rev = 0; a.X1 = nullptr; a.ld1 = 0; a.X2 = nullptr; a.ld2 = 0; a.X3 = nullptr; a.ld3 = 0; a.kreal = K; a.dbg = (int)dsh::switch_int(dsh::SW_TL_DBG);
    if (pro == 3) { a.ldx = 512; a.X1 = tcat[1]; a.ld1 = 256; a.X2 = tcat[2]; a.ld2 = 128; a.X3 = tcat[3]; a.ld3 = 128; a.kreal = frames; }
    if (raw && R && Cf && Ct && act == 0 && ((pro == 2 && K == 512) || (pro == 0 && K == 1024))) {
        // timing mode, DSH_HILO=1: the residual-carrying launch on hi / lo planes — R is taken as the hi plane, Cf's buffer as the lo plane (in / out)
        if (dsh::hilo_op()) { a.Rlo = Cf; a.Clo = Cf; a.Cf = nullptr; }
    }
    if (pro == 3 && raw) {     // timing mode: the caller's [Mp, 1024] buffer is cut into four segment buffers of the right sizes (contents are garbage anyway)
        const char* xb = reinterpret_cast<const char*>(X);
        a.X1 = xb + Mp * 512 * 2; a.X2 = xb + Mp * 768 * 2; a.X3 = frames > 896 ? xb + Mp * 896 * 2 : nullptr;
    }
    if (gen2 && (pro == 1 || pro == 3)) {
        if (fold_c) { a.bias = fold_d; a.row_const = fold_c; }
        else { a.bias = bias ? bias : gamma; a.row_const = gamma; }      // raw timing mode: any valid vectors
    }
    if (pro == 2 && !raw) {   // the kernel takes the folded coefficient table: fold a scratch copy of the caller's [scale | shift] rows
        void* fsc = nullptr;
        const size_t fbytes = (size_t)a.bmod * 2 * K * 4;
        if (int e = scratch.alloc(&fsc, fbytes)) return e;
        DSH_HIP_CHECK(hipMemcpyAsync(fsc, film, fbytes, hipMemcpyDeviceToDevice, s));
        if (int e = dsh::launch_film_fold(reinterpret_cast<float*>(fsc), 2 * K, a.bmod, 1, K, gamma, beta, s)) return e;
        a.film = reinterpret_cast<const float*>(fsc);
    }
    // bench hooks (per-call scratch like everything else; each reads back after a stream sync)
    unsigned long long *clk_dev = nullptr, *trace_dev = nullptr, *probe_dev = nullptr;
    const long clk_mode = dsh::switch_int(dsh::SW_TL_CLK);
    a.clk = nullptr;
    if (clk_mode) {
        if (int e = scratch.alloc(reinterpret_cast<void**>(&clk_dev), 32)) return e;
        a.clk = clk_dev;
    }
    const char* tr_e = dsh::switch_str(dsh::SW_TL_TRACE);        // block timeline -> file named by the variable
    a.trace = nullptr;
    const size_t nblk = (size_t)dsh::ceil_div(M, 128) * 64;          // upper bound on blocks (grid.x * grid.y)
    if (tr_e && *tr_e) {
        if (int e = scratch.words(&trace_dev, nblk * 4, s)) return e;
        a.trace = trace_dev;
    }
    const char* pb_e = dsh::switch_str(dsh::SW_TL_PROBE);        // per-block phase probe of the gen-2 kernels -> file
    const size_t npb = (size_t)dsh::ceil_div(M, 128);
    const bool probe = gen2 && pb_e && *pb_e;
    if (probe) {
        if (int e = scratch.words(&probe_dev, npb * 8, s)) return e;
        a.clk = probe_dev;
    }
    if (int e = gen2 ? dsh::launch_tl2_linear(a, pro, s) : dsh::launch_tl_linear(a, pro, s)) return e;
    if (probe) { if (int e = dump_tl_probe(pb_e, probe_dev, npb, 7, s)) return e; }
    if (a.trace) { if (int e = dump_tl_trace(tr_e, trace_dev, nblk, true, s)) return e; }
    if (clk_dev && !probe) {
        DSH_HIP_CHECK(hipStreamSynchronize(s));      // (the probe words are scratch of this call)
        if (clk_mode == 2) {   // 2: read back and print
            unsigned long long hv[4];
            DSH_HIP_CHECK(hipMemcpy(hv, clk_dev, 32, hipMemcpyDeviceToHost));
            fprintf(stderr, "[tl clock probe] block 0: %llu shader cycles in %.2f us -> %.3f GHz; barrier-parked cycles (wave 0) %llu\n", hv[0], hv[1] / 100.0, hv[0] / (hv[1] * 10.0), hv[2]);
        }
    }
    if (!raw) {
        if (hilo) { if (int e = dsh::launch_untile_rows_hilo(a.Ct, a.Clo, N, M, N, Cf, N, s)) return e; }
        else if (Cf) { if (int e = dsh::launch_untile_rows_f32(a.Cf, N, M, Cf, N, s)) return e; }
        if (Ct) { if (int e = dsh::launch_untile_rows_bf16(a.Ct, N, M, N, Ct, N, s)) return e; }
        DSH_HIP_CHECK(hipStreamSynchronize(s));      // the per-call scratch is released on return
    }
    return 0;
    API_END
}

int dsh_op_tl2_ffn(void* hip_stream, const void* X, const float* Hres, const void* W1, const float* b1, const void* W2, const float* b2,
                   const void* W3, const float* b3, const float* gamma, const float* beta, const float* film, int32_t frames, int32_t nb,
                   const float* row_const, int32_t n_const_rows, float* Cf, void* Ct, int32_t M) {
    API_BEGIN
    DSH_REQUIRE(X && Hres && W1 && b1 && W2 && b2 && W3 && b3 && gamma && beta && film && Cf && Ct && M > 0 && frames > 0 && nb > 0, "invalid argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    constexpr int D = 512, F = 1024;
    OpScratch scratch;
    // weight stream (see tl2.hip / Denoiser::layer_from): the pi-permuted rows of the PRODUCTION packer, from the caller's row-major bf16 weights
    const int ver = dsh::ffn_generation();            // 2: tl2_ffn_kernel, 3 (default): tl3_ffn_kernel (K-outer head of Linear3)
    constexpr size_t CH = 16384;
    std::vector<uint16_t> st((size_t)80 * CH), perm[3], frag;
    const void* wsrc[3] = {W1, W2, W3}; const int wn[3] = {F, D, D}, wk[3] = {D, F, D};
    DSH_HIP_CHECK(hipStreamSynchronize(s));
    for (int i = 0; i < 3; ++i) {
        std::vector<float> hw;
        if (int e = fetch_bf16_as_f32(hw, wsrc[i], (size_t)wn[i] * wk[i])) return e;
        perm[i].resize(hw.size()); frag.resize(hw.size());
        dsh::tl_pack_linear(hw.data(), nullptr, wn[i], wk[i], wk[i], nullptr, nullptr, perm[i].data(), frag.data(), nullptr, nullptr);
    }
    dsh::tl_pack_ffn_stream(ver, perm[0].data(), perm[1].data(), perm[2].data(), st.data());
    void *wst = nullptr, *tx = nullptr, *tr = nullptr, *tcf = nullptr, *tct = nullptr, *fsc = nullptr;
    const size_t Mp = (size_t)dsh::round_up(M, 128) + 128;
    if (int e = scratch.alloc(&wst, st.size() * 2)) return e;
    DSH_HIP_CHECK(hipMemcpy(wst, st.data(), st.size() * 2, hipMemcpyHostToDevice));
    if (int e = scratch.alloc(&tx, Mp * D * 2)) return e;
    if (int e = scratch.alloc(&tr, Mp * D * 4)) return e;
    if (int e = scratch.alloc(&tcf, Mp * D * 4)) return e;
    if (int e = scratch.alloc(&tct, Mp * D * 2)) return e;
    if (int e = dsh::launch_tile_rows_bf16<dsh::bf16>(reinterpret_cast<const dsh::bf16*>(X), D, M, D, tx, D, s)) return e;
    if (int e = dsh::launch_tile_rows_f32(Hres, D, M, reinterpret_cast<float*>(tr), D, s)) return e;
    const size_t fbytes = (size_t)nb * 2 * D * 4;
    if (int e = scratch.alloc(&fsc, fbytes)) return e;
    DSH_HIP_CHECK(hipMemcpyAsync(fsc, film, fbytes, hipMemcpyDeviceToDevice, s));
    if (int e = dsh::launch_film_fold(reinterpret_cast<float*>(fsc), 2 * D, nb, 1, D, gamma, beta, s)) return e;
    dsh::Tl2FfnArgs a;
    a.X = tx; a.Wffn = wst; a.b1 = b1; a.b2 = b2; a.b3 = b3; a.film = reinterpret_cast<const float*>(fsc); a.film_ld = 2 * D; a.film_off = 0;
    a.frames = frames; a.bmod = nb; a.half_row0 = 0x7fffffff; a.R = reinterpret_cast<const float*>(tr); a.Cf = reinterpret_cast<float*>(tcf);
    a.Ct = tct; a.row_const = row_const; a.n_const_rows = n_const_rows; a.M = M; a.trace = nullptr; a.clk = nullptr; a.rev = 0;
    a.Rhi = nullptr; a.Rlo = nullptr; a.Clo = nullptr;
    // DSH_HILO=1 (generation 3 only): residual stream as hi / lo planes — the residual of this call is split, Cf comes back as hi + lo
    const bool hilo = ver == 3 && dsh::hilo_op();
    void *trh = nullptr, *trl = nullptr, *tcl = nullptr;
    if (hilo) {
        if (int e = scratch.alloc(&trh, Mp * D * 2)) return e;
        if (int e = scratch.alloc(&trl, Mp * D * 2)) return e;
        if (int e = scratch.alloc(&tcl, Mp * D * 2)) return e;
        if (int e = dsh::launch_tile_rows_hilo(Hres, D, M, D, trh, trl, D, s)) return e;
        a.R = nullptr; a.Cf = nullptr; a.Rhi = trh; a.Rlo = trl; a.Clo = tcl;
        // DSH_FFN_X_IS_HI=1: the input IS the hi plane of the residual, as in the denoiser's layers (X is ignored) — the form
        // DSH_FFN_PC=3 keeps in registers
        if (dsh::switch_int(dsh::SW_FFN_X_IS_HI) != 0) a.X = trh;
    }
    // bench hooks: phase probe and block timeline, one slot per 128-token block
    unsigned long long *probe_dev = nullptr, *trace_dev = nullptr;
    const size_t nblk = (size_t)dsh::ceil_div(M, 128);
    const char* pb_e = dsh::switch_str(dsh::SW_TL_PROBE);
    if (pb_e && *pb_e) {
        if (int e = scratch.words(&probe_dev, nblk * 8, s)) return e;
        a.clk = probe_dev;
    }
    const char* tr_e = dsh::switch_str(dsh::SW_TL_TRACE);
    if (tr_e && *tr_e) {
        if (int e = scratch.words(&trace_dev, nblk * 4, s)) return e;
        a.trace = trace_dev;
    }
    const int reps = 1 + (int)dsh::switch_int(dsh::SW_FFN_REPEAT);     // bench only: launch the kernel this many extra times (results unchanged: R != Cf)
    for (int i = 0; i < reps; ++i) { if (int e = (ver == 3 ? dsh::launch_tl3_ffn(a, s) : dsh::launch_tl2_ffn(a, s))) return e; }
    if (a.trace) { if (int e = dump_tl_trace(tr_e, trace_dev, nblk, false, s)) return e; }
    if (a.clk) { if (int e = dump_tl_probe(pb_e, probe_dev, nblk, 8, s)) return e; }
    if (hilo) { if (int e = dsh::launch_untile_rows_hilo(a.Ct, a.Clo, D, M, D, Cf, D, s)) return e; }
    else if (int e = dsh::launch_untile_rows_f32(a.Cf, D, M, Cf, D, s)) return e;
    if (int e = dsh::launch_untile_rows_bf16(a.Ct, D, M, D, Ct, D, s)) return e;
    DSH_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
    API_END
}

// ---- fused front of the bf16 path (tl_aud.hip, tl_embed.hip): operands in natural order, built with the PRODUCTION packers.  What
// the launchers themselves refuse (null rows / outputs, ld_b, nf, row1) is passed through to them unchecked.
int dsh_op_tl_aud_tail(void* hip_stream, const void* Y, const float* X2, const float* ws1, const float* bs1, const float* w1, const float* b1,
                       const float* w2, const float* b2, const float* ws2, const float* bs2, const float* g1, const float* be1, const float* g2,
                       const float* be2, const float* film, int32_t frames, int32_t nb, int32_t Mc, float* out_f, void* out_b, int32_t ld_b) {
    API_BEGIN
    DSH_REQUIRE(ws1 && bs1 && w1 && b1 && w2 && b2 && ws2 && bs2 && g1 && be1 && g2 && be2 && film && nb > 0, "dsh_op_tl_aud_tail: null weight / FiLM operand");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    constexpr int DA = 128, F = 1024;
    OpScratch scratch;
    DSH_HIP_CHECK(hipStreamSynchronize(s));
    std::vector<float> hs1, h1, h2, hs2, bb, part, gg, be;
    if (int e = fetch_f32(hs1, ws1, (size_t)DA * DA)) return e;
    if (int e = fetch_f32(h1, w1, (size_t)F * DA)) return e;
    if (int e = fetch_f32(h2, w2, (size_t)DA * F)) return e;
    if (int e = fetch_f32(hs2, ws2, (size_t)DA * DA)) return e;
    std::vector<uint16_t> st((size_t)18 * 16384);
    dsh::tl_aud_pack_stream(hs1.data(), h1.data(), h2.data(), hs2.data(), st.data());
    // stacked biases [proj_out(sa) | linear1 | linear2 | proj_out(ffn)] and LayerNorm affines [block 1 | block 2], as Denoiser::finalize holds them
    const float* bsrc[4] = {bs1, b1, b2, bs2}; const int bn[4] = {DA, F, DA, DA};
    for (int i = 0; i < 4; ++i) { if (int e = fetch_f32(part, bsrc[i], bn[i])) return e; bb.insert(bb.end(), part.begin(), part.end()); }
    const float* gsrc[2] = {g1, g2}; const float* esrc[2] = {be1, be2};
    for (int i = 0; i < 2; ++i) {
        if (int e = fetch_f32(part, gsrc[i], DA)) return e; gg.insert(gg.end(), part.begin(), part.end());
        if (int e = fetch_f32(part, esrc[i], DA)) return e; be.insert(be.end(), part.begin(), part.end());
    }
    void *wst = nullptr, *dbias = nullptr, *dg = nullptr, *db = nullptr, *fsc = nullptr;
    if (int e = scratch.upload(&wst, st.data(), st.size() * 2)) return e;
    if (int e = scratch.upload(&dbias, bb.data(), bb.size() * 4)) return e;
    if (int e = scratch.upload(&dg, gg.data(), gg.size() * 4)) return e;
    if (int e = scratch.upload(&db, be.data(), be.size() * 4)) return e;
    const int film_ld = 4 * DA;
    const size_t fbytes = (size_t)nb * film_ld * 4;
    if (int e = scratch.alloc(&fsc, fbytes)) return e;
    DSH_HIP_CHECK(hipMemcpyAsync(fsc, film, fbytes, hipMemcpyDeviceToDevice, s));
    if (int e = dsh::launch_film_fold(reinterpret_cast<float*>(fsc), film_ld, nb, 2, DA, reinterpret_cast<const float*>(dg), reinterpret_cast<const float*>(db), s)) return e;
    const int rc = dsh::launch_tl_aud_tail(Y, X2, wst, reinterpret_cast<const float*>(dbias), reinterpret_cast<const float*>(fsc), film_ld, nb, frames, Mc,
                                           out_f, out_b, ld_b, s);
    DSH_HIP_CHECK(hipStreamSynchronize(s));      // the per-call scratch is released on return
    return rc;
    API_END
}

int dsh_op_tl_aproj(void* hip_stream, const void* X, const float* W, const float* bias, int32_t n_enc, void* out0, void* out1, int32_t Mc) {
    API_BEGIN
    DSH_REQUIRE(W && bias && (n_enc == 1 || n_enc == 2) && Mc > 0, "dsh_op_tl_aproj: null weight, or not one or two encoders");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    OpScratch scratch;
    DSH_HIP_CHECK(hipStreamSynchronize(s));
    std::vector<float> hw;
    if (int e = fetch_f32(hw, W, (size_t)n_enc * 256 * 256)) return e;
    std::vector<uint16_t> st((size_t)n_enc * 65536);
    for (int e = 0; e < n_enc; ++e) dsh::tl_aud_pack_audio_proj(hw.data() + (size_t)e * 65536, st.data() + (size_t)e * 65536);   // encoder e at + e * 128 KB
    void *wf = nullptr, *t0 = nullptr, *t1 = nullptr;
    if (int e = scratch.upload(&wf, st.data(), st.size() * 2)) return e;
    const size_t tbytes = (size_t)dsh::round_up(Mc, 32) * 256 * 2;       // tiled outputs: whole 32-row blocks (the kernel stores into the padding rows)
    if (out0) { if (int e = scratch.alloc(&t0, tbytes)) return e; }
    if (out1) { if (int e = scratch.alloc(&t1, tbytes)) return e; }
    int rc = dsh::launch_tl_aproj(X, wf, bias, n_enc, t0, t1, Mc, s);
    if (!rc) rc = dsh::launch_untile_rows_bf16(t0, 256, Mc, 256, out0, 256, s);
    if (!rc && n_enc == 2) rc = dsh::launch_untile_rows_bf16(t1, 256, Mc, 256, out1, 256, s);
    DSH_HIP_CHECK(hipStreamSynchronize(s));
    return rc;
    API_END
}

int dsh_op_tl_joint(void* hip_stream, const float* x, int32_t ldx, int32_t c0, int32_t w, const float* Wj, const float* bias, const float* pe,
                    int32_t frames, const float* cnull, int32_t Mc, int32_t row1, float* h_out) {
    API_BEGIN
    DSH_REQUIRE(x && Wj && h_out && w > 0 && c0 >= 0 && c0 + w <= ldx && Mc > 0, "dsh_op_tl_joint: null x / weight / output, or a channel slice outside the row");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    OpScratch scratch;
    DSH_HIP_CHECK(hipStreamSynchronize(s));
    const int nf = dsh::ceil_div(w, 16), Mp = dsh::round_up(Mc, 32);
    std::vector<float> hw;
    if (int e = fetch_f32(hw, Wj, (size_t)512 * w)) return e;
    std::vector<uint16_t> fr((size_t)512 * nf * 16);
    dsh::tl_joint_pack_weight(hw.data(), w, nf, fr.data());
    void *wf = nullptr, *xt = nullptr, *hi = nullptr, *lo = nullptr;
    if (int e = scratch.upload(&wf, fr.data(), fr.size() * 2)) return e;
    if (int e = scratch.alloc(&xt, (size_t)Mp * nf * 16 * 2)) return e;
    if (int e = dsh::launch_tile_rows_bf16<float>(x + c0, ldx, Mc, w, xt, nf * 16, s)) return e;      // as Denoiser::run_encoder does
    // planes: the null half's blocks at row 0, the conditional half's at row1 (CFG) — rows the kernel does not write come back as 0
    const int rows = (cnull ? std::max(row1, 0) : 0) + Mp;
    if (int e = scratch.alloc(&hi, (size_t)rows * 512 * 2)) return e;
    if (int e = scratch.alloc(&lo, (size_t)rows * 512 * 2)) return e;
    DSH_HIP_CHECK(hipMemsetAsync(hi, 0, (size_t)rows * 512 * 2, s));
    DSH_HIP_CHECK(hipMemsetAsync(lo, 0, (size_t)rows * 512 * 2, s));
    int rc = dsh::launch_tl_joint(xt, nf, wf, bias, pe, frames, cnull, Mc, row1, hi, lo, s);
    if (!rc) rc = dsh::launch_untile_rows_hilo(hi, lo, 512, rows, 512, h_out, 512, s);
    DSH_HIP_CHECK(hipStreamSynchronize(s));
    return rc;
    API_END
}

int dsh_op_cross_attention(void* hip_stream, const dsh_cross_attn_weights* w, const float* x, const float* xf, const float* emb,
                           int32_t B, int32_t T, int32_t N, int32_t D, int32_t L, int32_t E, int32_t num_head, float* y) {
    API_BEGIN
    DSH_REQUIRE(w && x && xf && emb && y && B > 0 && T > 0 && N > 0, "invalid argument");
    DSH_REQUIRE(D % 64 == 0 && L % 32 == 0 && E % 32 == 0 && num_head > 0 && D % num_head == 0, "cross_attention: D % 64, L % 32, E % 32");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    OpScratch scratch;
    auto salloc = [&](float** out, size_t n) -> int { return scratch.alloc(reinterpret_cast<void**>(out), n * sizeof(float)); };
    const int M = B * T, Mk = B * N;
    float *n1, *q, *nf, *kv, *att, *se, *film, *sy;
    if (int e = salloc(&n1, (size_t)M * D)) return e;
    if (int e = salloc(&q, (size_t)M * D)) return e;
    if (int e = salloc(&nf, (size_t)Mk * L)) return e;
    if (int e = salloc(&kv, (size_t)Mk * 2 * D)) return e;
    if (int e = salloc(&att, (size_t)M * D)) return e;
    if (int e = salloc(&se, (size_t)B * E)) return e;
    if (int e = salloc(&film, (size_t)B * 2 * D)) return e;
    if (int e = salloc(&sy, (size_t)M * D)) return e;
    auto gemm = [&](const float* A, int lda, const float* W, int K, const float* bias, int Mr, int Nc, const float* R, float* C, int ldc) -> int {
        dsh::GemmArgs a;
        a.A = A; a.lda = lda; a.W = W; a.ldw = K; a.bias = bias; a.R = R; a.ldr = ldc; a.res_mod = 0; a.Cf = C; a.ldcf = ldc;
        a.Ct = nullptr; a.ldct = 0; a.M = Mr; a.N = Nc; a.K = K; a.act = dsh::ACT_NONE; a.act_after_res = 0;
        return dsh::launch_gemm_f32(a, s);
    };
    // query = Wq LN(x); key | value = Wk | Wv text_norm(xf)                                     (transformer.py:151-161)
    if (int e = dsh::launch_ln_rows<float>(const_cast<float*>(x), D, M, D, nullptr, 0, w->norm_g, w->norm_b, n1, D, s)) return e;
    if (int e = gemm(n1, D, w->wq, D, w->bq, M, D, nullptr, q, D)) return e;
    if (int e = dsh::launch_ln_rows<float>(const_cast<float*>(xf), L, Mk, L, nullptr, 0, w->text_norm_g, w->text_norm_b, nf, L, s)) return e;
    if (int e = gemm(nf, L, w->wk, L, w->bk, Mk, D, nullptr, kv, 2 * D)) return e;
    if (int e = gemm(nf, L, w->wv, L, w->bv, Mk, D, nullptr, kv + D, 2 * D)) return e;
    if (int e = dsh::launch_linear_cross_attention(q, D, B, T, kv, 2 * D, N, D, D / num_head, att, D, s)) return e;
    // y = x + StylizationBlock(att, emb): emb_layers = SiLU -> Linear(E, 2D); LN * (1 + scale) + shift -> SiLU -> Linear  (:86-97, :165)
    if (int e = dsh::launch_silu_f32(emb, se, (size_t)B * E, s)) return e;
    if (int e = gemm(se, E, w->sty_emb_w, E, w->sty_emb_b, B, 2 * D, nullptr, film, 2 * D)) return e;
    if (int e = dsh::launch_ln_film_silu_rows<float, float>(att, D, M, D, w->sty_norm_g, w->sty_norm_b, film, 2 * D, 0, T, B, sy, D, s)) return e;
    if (int e = gemm(sy, D, w->sty_out_w, D, w->sty_out_b, M, D, x, y, D)) return e;
    DSH_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
    API_END
}

int dsh_op_linear_attention(void* hip_stream, const float* qkv, int32_t nb, int32_t frames, int32_t D, int32_t head_dim,
                            float* y) {
    API_BEGIN
    return dsh::launch_linear_attention<float>(qkv, 3 * D, nb, frames, D, head_dim, y, D, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

// the product kernel works on the tiled layout of the token-per-lane Linears: convert in scratch (test helper).
// The batch is split into two halves (nh clips, then the rest) with a block-aligned gap between them, like the CFG halves of the denoiser.
// rev: the kernel walks the clips in descending order (the denoiser's tl_block_index order); the result is the same, bit for bit.
static int attn_tiled_via_scratch(hipStream_t s, const void* qkv, int nb, int nh, int frames, int D, void* y, const int* lens, int rev = 0) {
    {
        const int M0 = nh * frames, r0 = dsh::round_up(M0, 128), M1 = (nb - nh) * frames;
        const size_t Mp = (size_t)r0 + dsh::round_up(M1 > 0 ? M1 : 1, 128) + 128;
        OpScratch scratch;
        void* sc[2] = {nullptr, nullptr};
        if (int e = scratch.alloc(&sc[0], Mp * 3 * D * 2)) return e;
        if (int e = scratch.alloc(&sc[1], Mp * D * 2)) return e;
        const dsh::bf16* q = reinterpret_cast<const dsh::bf16*>(qkv);
        char* tq = reinterpret_cast<char*>(sc[0]); char* ty = reinterpret_cast<char*>(sc[1]);
        if (int e = dsh::launch_tile_rows_bf16<dsh::bf16>(q, 3 * D, M0, 3 * D, tq, 3 * D, s)) return e;
        if (M1 > 0) { if (int e = dsh::launch_tile_rows_bf16<dsh::bf16>(q + (size_t)M0 * 3 * D, 3 * D, M1, 3 * D, tq + (size_t)r0 * 3 * D * 2, 3 * D, s)) return e; }
        if (int e = dsh::launch_linear_attention_tiled(tq, nb, nh, r0, frames, D, ty, s, rev, lens)) return e;
        if (int e = dsh::launch_untile_rows_bf16(ty, D, M0, D, y, D, s)) return e;
        if (M1 > 0) { if (int e = dsh::launch_untile_rows_bf16(ty + (size_t)r0 * D * 2, D, M1, D, reinterpret_cast<dsh::bf16*>(y) + (size_t)M0 * D, D, s)) return e; }
        DSH_HIP_CHECK(hipStreamSynchronize(s));      // the per-call scratch is released on return
        return 0;
    }
}

int dsh_op_linear_attention_bf16(void* hip_stream, const void* qkv, int32_t nb, int32_t frames, int32_t D, int32_t head_dim,
                                 void* y) {
    API_BEGIN
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    if (head_dim == 64 && frames <= 96) return attn_tiled_via_scratch(s, qkv, nb, (nb + 1) / 2, frames, D, y, nullptr);
    return dsh::launch_linear_attention<dsh::bf16>(reinterpret_cast<const dsh::bf16*>(qkv), 3 * D, nb, frames, D, head_dim,
                                                   reinterpret_cast<dsh::bf16*>(y), D, s);
    API_END
}

int dsh_op_linear_attention_ragged(void* hip_stream, int32_t dtype, int32_t variant, const void* qkv, int32_t nb, int32_t frames, int32_t D,
                                   int32_t head_dim, void* y, const int32_t* lens_dev, int32_t n_lens, const float* film) {
    API_BEGIN
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    DSH_REQUIRE(qkv && y && nb > 0 && frames > 0 && (dtype == 0 || dtype == 1) && variant >= 0 && variant <= 2, "linear_attention_ragged: invalid argument");
    DSH_REQUIRE(!lens_dev || (n_lens > 0 && (nb == n_lens || nb == 2 * n_lens)), "linear_attention_ragged: nb must be n_lens or 2 * n_lens (CFG-doubled)");
    const int lm = lens_dev ? n_lens : nb;
    if (variant == 2) {
        DSH_REQUIRE(dtype == 0 && film, "linear_attention_ragged: variant 2 is the fp32 kernel with the StylizationBlock front (needs film)");
        return dsh::launch_linear_attention_sty_f32(reinterpret_cast<const float*>(qkv), 3 * D, nb, frames, D, reinterpret_cast<float*>(y), D, film, 2 * D, 0, lm, s,
                                                    lens_dev, lm);
    }
    if (dtype == 0)
        return dsh::launch_linear_attention<float>(reinterpret_cast<const float*>(qkv), 3 * D, nb, frames, D, head_dim, reinterpret_cast<float*>(y), D, s, lens_dev, lm);
    if (variant == 0 && head_dim == 64 && frames <= 96) return attn_tiled_via_scratch(s, qkv, nb, lm, frames, D, y, lens_dev);
    return dsh::launch_linear_attention<dsh::bf16>(reinterpret_cast<const dsh::bf16*>(qkv), 3 * D, nb, frames, D, head_dim,
                                                   reinterpret_cast<dsh::bf16*>(y), D, s, lens_dev, lm);
    API_END
}

int dsh_op_linear_attention_tiled(void* hip_stream, const void* qkv, int32_t nb, int32_t n_half, int32_t frames, int32_t D, void* y,
                                  const int32_t* lens_dev, int32_t n_lens, int32_t rev) {
    API_BEGIN
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    DSH_REQUIRE(qkv && y && nb > 0 && n_half > 0 && n_half <= nb && frames > 0 && frames <= 96 && D > 0 && D % 64 == 0 && (rev == 0 || rev == 1),
                "linear_attention_tiled: invalid argument (64-channel heads, <= 96 frames, 0 < n_half <= nb, rev 0 or 1)");
    // (the kernel reads lens[b] in the first half and lens[b - n_half] in the second: the halves must be the CFG halves of the same clips)
    DSH_REQUIRE(!lens_dev || (n_lens == n_half && (nb == n_lens || nb == 2 * n_lens)), "linear_attention_tiled: with lengths n_half = n_lens and nb = n_lens or 2 * n_lens");
    return attn_tiled_via_scratch(s, qkv, nb, n_half, frames, D, y, lens_dev, rev);
    API_END
}

int dsh_op_layernorm(void* hip_stream, const float* x, int32_t M, int32_t D, const float* gamma, const float* beta,
                     float* out) {
    API_BEGIN
    // ln_rows takes a mutable residual stream (it can fold a constant in); with pre_add == null it only reads
    return dsh::launch_ln_rows<float>(const_cast<float*>(x), D, M, D, nullptr, 0, gamma, beta, out, D,
                                      reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_interp_time(void* hip_stream, const float* x, int32_t batch, int32_t frames_in, int32_t channels, float* y,
                    int32_t frames_out) {
    API_BEGIN
    DSH_REQUIRE(x && y, "null pointer");
    return dsh::launch_interp_time(x, batch, frames_in, channels, y, frames_out, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_interp_time_ragged(void* hip_stream, const float* x, int32_t batch, int32_t frames_in, int32_t channels, float* y, int32_t frames_out,
                           const int32_t* lens_in_dev, const int32_t* lens_out_dev) {
    API_BEGIN
    return dsh::launch_interp_time_ragged(x, batch, frames_in, channels, y, frames_out, lens_in_dev, lens_out_dev, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_inv_standardize(void* hip_stream, const float* x, int64_t n, int32_t channels, const float* mean, const float* stdv,
                        float* y) {
    API_BEGIN
    DSH_REQUIRE(x && y && mean && stdv && n >= 0 && channels > 0, "invalid argument");
    return dsh::launch_affine_cols(x, (size_t)n, channels, mean, stdv, y, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

static int check_rotation_args(const char* what, const void* x, int64_t ld_x, int64_t rows, int32_t joints, const void* m0, const void* s0,
                               const void* m1, const void* s1, const int32_t* lengths_dev, int32_t frames) {
    DSH_REQUIRE(joints >= 1, std::string(what) + ": joints must be at least 1");
    DSH_REQUIRE(ld_x >= 3 * (int64_t)joints, std::string(what) + ": input stride below 3 * joints");
    DSH_REQUIRE(m0 && s0 && m1 && s1, std::string(what) + ": null statistics pointer");
    DSH_REQUIRE(x && rows >= 0, std::string(what) + ": null input or negative row count");
    DSH_REQUIRE(!lengths_dev || (frames >= 1 && rows % frames == 0), std::string(what) + ": lengths need frames >= 1 dividing rows");
    return 0;
}

int dsh_axis_angle_to_euler(void* hip_stream, const float* x, int64_t ld_x, int64_t rows, int32_t joints, const float* mean_aa,
                            const float* std_aa, const float* mean_e, const float* std_e, float* y_std, int64_t ld_std, float* y_deg,
                            int64_t ld_deg, const int32_t* lengths_dev, int32_t frames) {
    API_BEGIN
    if (int e = check_rotation_args("dsh_axis_angle_to_euler", x, ld_x, rows, joints, mean_aa, std_aa, mean_e, std_e, lengths_dev, frames)) return e;
    DSH_REQUIRE(y_std || y_deg, "dsh_axis_angle_to_euler: both outputs null");
    DSH_REQUIRE((!y_std || ld_std >= 3 * (int64_t)joints) && (!y_deg || ld_deg >= 3 * (int64_t)joints),
                "dsh_axis_angle_to_euler: output stride below 3 * joints");
    return dsh::launch_axis_angle_to_euler(x, ld_x, rows, joints, mean_aa, std_aa, mean_e, std_e, y_std, ld_std, y_deg, ld_deg, lengths_dev,
                                           frames, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_euler_to_axis_angle(void* hip_stream, const float* x, int64_t ld_x, int64_t rows, int32_t joints, const float* mean_e,
                            const float* std_e, const float* mean_aa, const float* std_aa, float* y, int64_t ld_y,
                            const int32_t* lengths_dev, int32_t frames) {
    API_BEGIN
    if (int e = check_rotation_args("dsh_euler_to_axis_angle", x, ld_x, rows, joints, mean_e, std_e, mean_aa, std_aa, lengths_dev, frames)) return e;
    DSH_REQUIRE(y, "dsh_euler_to_axis_angle: both outputs null (there is one)");
    DSH_REQUIRE(ld_y >= 3 * (int64_t)joints, "dsh_euler_to_axis_angle: output stride below 3 * joints");
    return dsh::launch_euler_to_axis_angle(x, ld_x, rows, joints, mean_e, std_e, mean_aa, std_aa, y, ld_y, lengths_dev, frames,
                                           reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

// what the two forward-kinematics calls share, checked before any launch
static int check_fk_args(const char* what, const float* x, int64_t ld_x, int64_t rows, int32_t kind, const float* mean, const float* stdv,
                         int32_t joints, int32_t channels, const int32_t* parents, const float* offsets, const int32_t* channel_joint,
                         const float* rest_rot, const int32_t* joint_channel, const int32_t* lengths_dev, int32_t frames) {
    DSH_REQUIRE(joints >= 1 && joints <= DSH_FK_MAX_JOINTS, std::string(what) + ": joints outside 1 .. 256");
    DSH_REQUIRE(channels >= 1 && channels <= joints, std::string(what) + ": channel triples outside 1 .. joints");
    DSH_REQUIRE(kind == 0 || kind == 1, std::string(what) + ": input kind must be 0 (axis-angle) or 1 (Euler)");
    DSH_REQUIRE(x && mean && stdv && rows >= 0, std::string(what) + ": null input or statistics pointer, or negative row count");
    DSH_REQUIRE(parents && offsets && channel_joint && rest_rot && joint_channel, std::string(what) + ": null skeleton pointer");
    DSH_REQUIRE(ld_x >= 3 * (int64_t)channels, std::string(what) + ": input stride below 3 * channels");
    DSH_REQUIRE(!lengths_dev || (frames >= 1 && rows % frames == 0), std::string(what) + ": lengths need frames >= 1 dividing rows");
    return 0;
}

int dsh_fk_positions(void* hip_stream, const float* x, int64_t ld_x, int64_t rows, int32_t kind, const float* mean, const float* stdv,
                     int32_t joints, int32_t channels, const int32_t* parents, const float* offsets, const int32_t* channel_joint,
                     const float* rest_rot, const int32_t* joint_channel, float* pos, int64_t ld_pos, float* wrot, int64_t ld_wrot,
                     const int32_t* lengths_dev, int32_t frames) {
    API_BEGIN
    if (int e = check_fk_args("dsh_fk_positions", x, ld_x, rows, kind, mean, stdv, joints, channels, parents, offsets, channel_joint, rest_rot,
                              joint_channel, lengths_dev, frames)) return e;
    DSH_REQUIRE(pos, "dsh_fk_positions: null position output");
    DSH_REQUIRE(ld_pos >= 3 * (int64_t)joints, "dsh_fk_positions: position stride below 3 * joints");
    DSH_REQUIRE(!wrot || ld_wrot >= 9 * (int64_t)joints, "dsh_fk_positions: rotation stride below 9 * joints");
    const dsh::FkSkeleton sk{joints, channels, parents, offsets, channel_joint, rest_rot, joint_channel};
    return dsh::launch_fk_positions(x, ld_x, rows, kind, mean, stdv, sk, pos, ld_pos, wrot, ld_wrot, lengths_dev, frames,
                                    reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_fk_positions_vjp(void* hip_stream, const float* x, int64_t ld_x, int64_t rows, int32_t kind, const float* mean, const float* stdv,
                         int32_t joints, int32_t channels, const int32_t* parents, const float* offsets, const int32_t* channel_joint,
                         const float* rest_rot, const int32_t* joint_channel, const float* g, int64_t ld_g, float* dx, int64_t ld_dx,
                         const int32_t* lengths_dev, int32_t frames) {
    API_BEGIN
    if (int e = check_fk_args("dsh_fk_positions_vjp", x, ld_x, rows, kind, mean, stdv, joints, channels, parents, offsets, channel_joint,
                              rest_rot, joint_channel, lengths_dev, frames)) return e;
    DSH_REQUIRE(kind == 0, "dsh_fk_positions_vjp: the gradient is built for axis-angle input only");
    DSH_REQUIRE(g && dx, "dsh_fk_positions_vjp: null gradient pointer");
    DSH_REQUIRE(ld_g >= 3 * (int64_t)joints, "dsh_fk_positions_vjp: gradient stride below 3 * joints");
    DSH_REQUIRE(ld_dx >= 3 * (int64_t)channels, "dsh_fk_positions_vjp: output stride below 3 * channels");
    const dsh::FkSkeleton sk{joints, channels, parents, offsets, channel_joint, rest_rot, joint_channel};
    return dsh::launch_fk_positions_vjp(x, ld_x, rows, mean, stdv, sk, g, ld_g, dx, ld_dx, lengths_dev, frames,
                                        reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

// what the three step ops share, checked, as the eta = 0 step without saved noisy tails; each entry adds what is its own
static int step_args(const std::string& what, dsh::DdimStepArgs& a, float* x, const float* eps, float* x0_out, const float* gt, const uint8_t* mask,
                     const float* noise2, int32_t B, int32_t frames, int32_t channels, float c1, float c2, float sqrt_ab_prev, float sqrt_1m_ab_prev,
                     int32_t overlap_len, int32_t blend, int32_t tail_blend, int32_t clip, int32_t c_lo, int32_t c_hi) {
    DSH_REQUIRE(x && eps && B > 0 && frames > 0 && channels > 0, "invalid argument");
    DSH_REQUIRE(!mask || (gt && noise2), what + ": a mask needs gt and noise2");
    DSH_REQUIRE(overlap_len >= 0 && overlap_len <= frames, what + ": 0 <= overlap_len <= frames");
    DSH_REQUIRE(!tail_blend || 2 * (int64_t)overlap_len <= frames, what + ": tail_blend needs 2 * overlap_len <= frames");
    DSH_REQUIRE(c_lo >= 0 && c_hi <= channels, what + ": channel range outside [0, channels]");
    a.x = x; a.eps = eps; a.x0_out = x0_out; a.c1 = c1; a.c2 = c2; a.sqrt_ab_prev = sqrt_ab_prev; a.sqrt_1m_ab_prev = sqrt_1m_ab_prev;
    a.coef_eps = sqrt_1m_ab_prev; a.sigma = 0.f; a.noise1 = nullptr;
    a.mask = mask; a.gt = gt; a.noise2 = noise2; a.blend = (mask && blend) ? 1 : 0; a.tail_blend = (a.blend && tail_blend) ? 1 : 0;
    a.clip = clip; a.overlap_len = overlap_len; a.frames = frames; a.channels = channels; a.n = (size_t)B * frames * channels;
    a.tail_in = nullptr; a.tail_out = nullptr; a.c_lo = c_lo; a.c_hi = c_hi;
    return 0;
}

int dsh_op_ddim_step(void* hip_stream, float* x, const float* eps, const float* gt, const uint8_t* mask, const float* noise2,
                     int32_t B, int32_t frames, int32_t channels, float c1, float c2, float sqrt_ab_prev, float sqrt_1m_ab_prev,
                     int32_t overlap_len, int32_t blend, int32_t tail_blend, int32_t clip, int32_t c_lo, int32_t c_hi) {
    API_BEGIN
    dsh::DdimStepArgs a;
    if (int e = step_args("ddim_step", a, x, eps, nullptr, gt, mask, noise2, B, frames, channels, c1, c2, sqrt_ab_prev, sqrt_1m_ab_prev, overlap_len,
                          blend, tail_blend, clip, c_lo, c_hi)) return e;
    return dsh::launch_ddim_step(a, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_philox_randn(void* hip_stream, float* out, int64_t n, uint64_t seed, uint64_t offset) {
    API_BEGIN
    DSH_REQUIRE(out && n >= 0, "invalid argument");
    return dsh::launch_philox_randn(out, (size_t)n, seed, offset, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_philox_randn_rows(void* hip_stream, float* out, int32_t rows, int64_t n_row, uint64_t seed, uint64_t offset,
                             const uint64_t* row_keys_host) {
    API_BEGIN
    DSH_REQUIRE(out && rows > 0 && n_row > 0 && row_keys_host, "invalid argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    uint64_t* kd = nullptr;
    DSH_HIP_CHECK(hipMalloc((void**)&kd, (size_t)rows * sizeof(uint64_t)));
    hipError_t ce = hipMemcpyAsync(kd, row_keys_host, (size_t)rows * sizeof(uint64_t), hipMemcpyHostToDevice, s);
    int rc = ce == hipSuccess ? dsh::launch_philox_randn_rows(out, rows, (size_t)n_row, seed, offset, kd, s) : -2;
    const hipError_t se = hipStreamSynchronize(s);   // the key array is released on return; an asynchronous kernel fault surfaces here
    (void)hipFree(kd);
    if (ce != hipSuccess) dsh::set_last_error(std::string("hipMemcpyAsync failed: ") + hipGetErrorString(ce));
    else if (se != hipSuccess) { dsh::set_last_error(std::string("philox_randn_rows: hipStreamSynchronize failed: ") + hipGetErrorString(se)); if (rc == 0) rc = -2; }
    return rc;
    API_END
}

// ---- one entry per small kernel of the sampler and around the denoiser (test helpers; include/diffsheg_hip.h) -------
int dsh_op_philox_randn_rows_ragged(void* hip_stream, float* out, int32_t rows, int64_t n_row, uint64_t seed, uint64_t offset,
                                    const uint64_t* row_keys_host, const int32_t* row_lens_host, uint64_t draw, int32_t channels) {
    API_BEGIN
    DSH_REQUIRE(out && rows > 0 && n_row > 0 && row_keys_host, "invalid argument");
    if (row_lens_host)
        for (int b = 0; b < rows; ++b)
            DSH_REQUIRE(row_lens_host[b] >= 0 && channels > 0 && (int64_t)row_lens_host[b] * channels <= n_row, "philox_randn_rows_ragged: a row length outside its row");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    OpScratch scratch;
    void *kd = nullptr, *ld = nullptr;
    if (int e = scratch.upload(&kd, row_keys_host, (size_t)rows * sizeof(uint64_t))) return e;
    if (row_lens_host) { if (int e = scratch.upload(&ld, row_lens_host, (size_t)rows * sizeof(int32_t))) return e; }
    const int rc = dsh::launch_philox_randn_rows(out, rows, (size_t)n_row, seed, offset, reinterpret_cast<const uint64_t*>(kd), s,
                                                 reinterpret_cast<const int*>(ld), draw, channels);
    DSH_HIP_CHECK(hipStreamSynchronize(s));          // the scratch arrays are released on return
    return rc;
    API_END
}

int dsh_op_philox_randn_rows_seeded(void* hip_stream, float* out, int32_t rows, int64_t n_row, uint64_t seed, uint64_t offset,
                                    const uint64_t* row_keys_host, const uint64_t* row_seeds_dev) {
    return dsh_op_philox_randn_rows_ragged_seeded(hip_stream, out, rows, n_row, seed, offset, row_keys_host, nullptr, 0, 0, row_seeds_dev);
}

int dsh_op_philox_randn_rows_ragged_seeded(void* hip_stream, float* out, int32_t rows, int64_t n_row, uint64_t seed, uint64_t offset,
                                           const uint64_t* row_keys_host, const int32_t* row_lens_host, uint64_t draw, int32_t channels,
                                           const uint64_t* row_seeds_dev) {
    API_BEGIN
    DSH_REQUIRE(out && rows > 0 && n_row > 0 && row_keys_host, "invalid argument");
    if (row_lens_host)
        for (int b = 0; b < rows; ++b)
            DSH_REQUIRE(row_lens_host[b] >= 0 && channels > 0 && (int64_t)row_lens_host[b] * channels <= n_row, "philox_randn_rows_ragged_seeded: a row length outside its row");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    OpScratch scratch;
    void *kd = nullptr, *ld = nullptr;
    if (int e = scratch.upload(&kd, row_keys_host, (size_t)rows * sizeof(uint64_t))) return e;
    if (row_lens_host) { if (int e = scratch.upload(&ld, row_lens_host, (size_t)rows * sizeof(int32_t))) return e; }
    const int rc = dsh::launch_philox_randn_rows(out, rows, (size_t)n_row, seed, offset, reinterpret_cast<const uint64_t*>(kd), s,
                                                 reinterpret_cast<const int*>(ld), draw, channels, row_seeds_dev);
    DSH_HIP_CHECK(hipStreamSynchronize(s));          // the scratch arrays are released on return
    return rc;
    API_END
}

// q_sample as an op: noise given, or (noise null) drawn in the pass with the addressing of dsh_op_philox_randn (row_keys_host null) /
// dsh_op_philox_randn_rows[_ragged][_seeded]
int dsh_op_q_sample(void* hip_stream, float* out, const float* x0, const float* noise, const float* a_dev, const float* s_dev, int32_t B,
                    int32_t frames, int32_t channels, int32_t c_lo, int32_t c_hi, int32_t fixed_from, uint64_t seed, uint64_t offset,
                    const uint64_t* row_keys_host, const uint64_t* row_seeds_dev, const int32_t* row_lens_host, uint64_t draw) {
    API_BEGIN
    DSH_REQUIRE(out && x0 && a_dev && s_dev && B > 0 && frames > 0 && channels > 0, "q_sample: invalid argument");
    DSH_REQUIRE(c_lo >= 0 && c_hi <= channels, "q_sample: channel range outside [0, channels]");
    DSH_REQUIRE(fixed_from >= -1 && fixed_from <= channels, "q_sample: fixed_from outside -1 .. channels");
    DSH_REQUIRE(noise || row_keys_host || (!row_seeds_dev && !row_lens_host), "q_sample: row seeds and row lengths of a Philox draw need the row keys");
    const size_t row_n = (size_t)frames * channels;
    DSH_REQUIRE(noise || !row_keys_host || row_n % 4 == 0, "q_sample: row keys need frames * channels to be a multiple of 4");
    if (row_lens_host)
        for (int b = 0; b < B; ++b) {
            DSH_REQUIRE(row_lens_host[b] >= 0 && row_lens_host[b] <= frames, "q_sample: a row length outside 0 .. frames");
            DSH_REQUIRE(noise || ((int64_t)row_lens_host[b] * channels) % 4 == 0, "q_sample: length * channels must be a multiple of 4 for every row of a Philox draw");
        }
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    OpScratch scratch;
    void *kd = nullptr, *ld = nullptr;
    if (!noise && row_keys_host) { if (int e = scratch.upload(&kd, row_keys_host, (size_t)B * sizeof(uint64_t))) return e; }
    if (row_lens_host) { if (int e = scratch.upload(&ld, row_lens_host, (size_t)B * sizeof(int32_t))) return e; }
    dsh::QSampleArgs a{};
    a.out = out; a.x0 = x0; a.noise = noise; a.a = a_dev; a.s = s_dev; a.n = (size_t)B * row_n; a.frames = frames; a.channels = channels;
    a.c_lo = c_lo; a.c_hi = c_hi; a.fixed_from = fixed_from;
    a.seed = seed; a.offset = offset; a.row_keys = reinterpret_cast<const uint64_t*>(kd); a.row_quads = kd ? row_n / 4 : 1;
    a.row_lens = reinterpret_cast<const int*>(ld); a.draw = draw; a.row_seeds = kd ? row_seeds_dev : nullptr;
    const int rc = dsh::launch_q_sample(a, s);
    if (kd || ld) DSH_HIP_CHECK(hipStreamSynchronize(s));          // the scratch arrays are released on return
    return rc;
    API_END
}

// keep mask of an edit (glue.edit_region): the host copies are validated here, the kernel reads the device copies
int dsh_op_region_mask(void* hip_stream, const int32_t* frames_host, const int32_t* frames_dev, int32_t nf, const int32_t* cols_host,
                       const int32_t* cols_dev, int32_t nc, int32_t B, int32_t T, int32_t C, uint8_t* keep) {
    API_BEGIN
    DSH_REQUIRE(B > 0 && T > 0 && C > 0 && nf >= 0 && nc >= 0 && keep, "region_mask: invalid argument");
    DSH_REQUIRE((nf == 0 || (frames_host && frames_dev)) && (nc == 0 || (cols_host && cols_dev)), "region_mask: ranges need their host and their device copy");
    for (int64_t i = 0; i < (int64_t)B * nf; ++i)
        DSH_REQUIRE(frames_host[2 * i] >= 0 && frames_host[2 * i] <= frames_host[2 * i + 1] && frames_host[2 * i + 1] <= T, "region_mask: a frame range outside 0 <= lo <= hi <= T");
    for (int i = 0; i < nc; ++i)
        DSH_REQUIRE(cols_host[2 * i] >= 0 && cols_host[2 * i] <= cols_host[2 * i + 1] && cols_host[2 * i + 1] <= C, "region_mask: a column range outside 0 <= lo <= hi <= C");
    return dsh::launch_region_mask(frames_dev, nf, cols_dev, nc, B, T, C, keep, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

// ---- window hand-off of live chains (streaming.py: StreamPool) ----------------------------------
namespace {
// the host copy of a slot index list: every entry inside the table and, where rows are written, no slot twice
int check_slots(const int32_t* slot_idx_host, int32_t R, int32_t S, bool distinct, const char* what) {
    DSH_REQUIRE(R == 0 || slot_idx_host, std::string(what) + ": the host copy of the slot indices is required");
    for (int r = 0; r < R; ++r) {
        DSH_REQUIRE(slot_idx_host[r] >= 0 && slot_idx_host[r] < S, std::string(what) + ": slot index outside the table");
        if (distinct)
            for (int q = 0; q < r; ++q) DSH_REQUIRE(slot_idx_host[q] != slot_idx_host[r], std::string(what) + ": a slot is written twice");
    }
    return 0;
}
}  // namespace

int dsh_op_chain_handoff(void* hip_stream, const float* tails, int32_t S, const int32_t* slot_idx_host, const int32_t* slot_idx_dev,
                         int32_t R, int32_t T, int32_t L, int32_t C, float* gt, uint8_t* mask) {
    API_BEGIN
    DSH_REQUIRE(R >= 0 && S > 0, "chain_handoff: invalid argument");
    if (int e = check_slots(slot_idx_host, R, S, false, "chain_handoff")) return e;
    return dsh::launch_chain_handoff(tails, S, slot_idx_dev, R, T, L, C, gt, mask, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_chain_save_tail(void* hip_stream, const float* x, const int32_t* lens_host, const int32_t* lens_dev, const int32_t* slot_idx_host,
                           const int32_t* slot_idx_dev, int32_t R, int32_t T, int32_t L, int32_t C, float* tails, int32_t S) {
    API_BEGIN
    DSH_REQUIRE(R >= 0 && S > 0, "chain_save_tail: invalid argument");
    DSH_REQUIRE((lens_host == nullptr) == (lens_dev == nullptr), "chain_save_tail: per-row lengths need their host and their device copy");
    if (int e = check_slots(slot_idx_host, R, S, true, "chain_save_tail")) return e;
    if (lens_host)
        for (int r = 0; r < R; ++r) DSH_REQUIRE(lens_host[r] >= L && lens_host[r] <= T, "chain_save_tail: a row length outside overlap_len .. frames");
    return dsh::launch_chain_save_tail(x, lens_dev, slot_idx_dev, S, R, T, L, C, tails, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

// synchronised window batches: the host copies are validated here (check_window_sync), the kernel reads the device copies
int dsh_op_window_sync(void* hip_stream, float* x, int32_t B, int32_t frames, int32_t channels, const int32_t* left_host, const int32_t* left_dev,
                       const int32_t* lens_host, const int32_t* lens_dev, int32_t L, int32_t c_lo, int32_t c_hi) {
    API_BEGIN
    DSH_REQUIRE(x && B > 0 && frames > 0 && channels > 0, "window_sync: invalid argument");
    DSH_REQUIRE(left_host && left_dev, "window_sync: the left neighbours need their host and their device copy");
    DSH_REQUIRE((lens_host == nullptr) == (lens_dev == nullptr), "window_sync: per-row lengths need their host and their device copy");
    std::string err;
    if (dsh::check_window_sync(left_host, lens_host, B, frames, L, err)) { dsh::set_last_error(err); return -1; }
    return dsh::launch_window_sync(x, B, frames, channels, left_dev, lens_dev, L, c_lo, c_hi, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_ddim_step_full(void* hip_stream, float* x, const float* eps, float* x0_out, const float* gt, const uint8_t* mask, const float* noise2,
                          const float* noise1, const float* tail_in, float* tail_out, int32_t B, int32_t frames, int32_t channels, float c1,
                          float c2, float sqrt_ab_prev, float sqrt_1m_ab_prev, float coef_eps, float sigma, int32_t overlap_len, int32_t blend,
                          int32_t tail_blend, int32_t clip, int32_t c_lo, int32_t c_hi) {
    API_BEGIN
    dsh::DdimStepArgs a;
    if (int e = step_args("ddim_step", a, x, eps, x0_out, gt, mask, noise2, B, frames, channels, c1, c2, sqrt_ab_prev, sqrt_1m_ab_prev, overlap_len,
                          blend, tail_blend, clip, c_lo, c_hi)) return e;
    DSH_REQUIRE(!tail_in || mask, "ddim_step: tail_in replaces the noised gt of a masked step (needs a mask)");
    a.coef_eps = coef_eps; a.sigma = sigma; a.noise1 = noise1; a.tail_in = tail_in; a.tail_out = tail_out;
    return dsh::launch_ddim_step(a, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_dpm2m_step(void* hip_stream, float* x, const float* eps, float* x0_prev, const float* gt, const uint8_t* mask, const float* noise2,
                      int32_t B, int32_t frames, int32_t channels, float c1, float c2, float sqrt_ab_prev, float sqrt_1m_ab_prev, float A, float Bc,
                      float G, int32_t second_order, int32_t overlap_len, int32_t blend, int32_t tail_blend, int32_t clip, int32_t c_lo, int32_t c_hi) {
    API_BEGIN
    DSH_REQUIRE(x0_prev, "invalid argument");
    dsh::DdimStepArgs a;
    if (int e = step_args("dpm2m_step", a, x, eps, x0_prev, gt, mask, noise2, B, frames, channels, c1, c2, sqrt_ab_prev, sqrt_1m_ab_prev, overlap_len,
                          blend, tail_blend, clip, c_lo, c_hi)) return e;
    // (the first-order form is the DDIM step at eta = 0, with its x0 left in the history)
    a.second = second_order ? 1 : 0; a.A = A; a.Bc = Bc; a.G = G;
    return dsh::launch_ddim_step(a, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_ddpm_step(void* hip_stream, float* x, const float* eps, const float* noise, float* x0_out, int64_t n, float c1, float c2, float coef1,
                     float coef2, float sigma, int32_t clip, int32_t channels, int32_t c_lo, int32_t c_hi) {
    API_BEGIN
    DSH_REQUIRE(x && eps && noise && n >= 0, "invalid argument");
    DSH_REQUIRE(c_hi <= c_lo || (channels > 0 && c_lo >= 0 && c_hi <= channels), "ddpm_step: a channel range needs the channel count and must lie inside it");
    dsh::DdpmStepArgs a;
    a.x = x; a.eps = eps; a.noise = noise; a.x0_out = x0_out; a.c1 = c1; a.c2 = c2; a.coef1 = coef1; a.coef2 = coef2; a.sigma = sigma;
    a.clip = clip; a.n = (size_t)n; a.channels = channels; a.c_lo = c_lo; a.c_hi = c_hi;
    return dsh::launch_ddpm_step(a, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

// dsh_guide -> dsh::GuideArgs, with the per-clip lengths checked on the host before any address is formed from them
static int guide_args(const std::string& what, const dsh_guide* g, int32_t B, int32_t frames, dsh::GuideArgs& ga) {
    DSH_REQUIRE(g, what + ": null guide");
    DSH_REQUIRE((g->lens_dev == nullptr) == (g->lens_host == nullptr), what + ": per-clip lengths need the host and the device copy");
    for (int b = 0; g->lens_host && b < B; ++b)
        DSH_REQUIRE(g->lens_host[b] >= 1 && g->lens_host[b] <= frames, what + ": a clip length outside 1 .. frames");
    ga.target = g->target; ga.weight = g->weight; ga.vel = g->vel; ga.acc = g->acc; ga.lens = g->lens_dev; ga.scale = g->scale; ga.space = g->space;
    return 0;
}

int dsh_op_guidance_grad(void* hip_stream, const float* z, float* g, int32_t B, int32_t frames, int32_t channels, int32_t c_lo, int32_t c_hi,
                         const dsh_guide* guide) {
    API_BEGIN
    DSH_REQUIRE(z && g && B > 0 && frames > 0 && channels > 0, "invalid argument");
    dsh::GuideArgs ga;
    if (int e = guide_args("guidance_grad", guide, B, frames, ga)) return e;
    ga.space = dsh::GUIDE_XT;
    return dsh::launch_guidance_grad(z, g, B, frames, channels, c_lo, c_hi, ga, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_guided_ddim_step(void* hip_stream, float* x, const float* eps, float* x0_out, const float* gt, const uint8_t* mask, const float* noise2,
                            const float* noise1, const dsh_guide* guide, int32_t B, int32_t frames, int32_t channels, float c1, float c2,
                            float sqrt_ab_prev, float sqrt_1m_ab_prev, float coef_eps, float sigma, float sqrt_1m_ab, float A, float Bc, float G,
                            int32_t second_order, int32_t overlap_len, int32_t blend, int32_t tail_blend, int32_t clip, int32_t c_lo, int32_t c_hi) {
    API_BEGIN
    dsh::DdimStepArgs a;
    if (int e = step_args("guided_ddim_step", a, x, eps, x0_out, gt, mask, noise2, B, frames, channels, c1, c2, sqrt_ab_prev, sqrt_1m_ab_prev,
                          overlap_len, blend, tail_blend, clip, c_lo, c_hi)) return e;
    dsh::GuideArgs ga;
    if (int e = guide_args("guided_ddim_step", guide, B, frames, ga)) return e;
    ga.sqrt_1m_ab = sqrt_1m_ab;
    if (second_order) { a.second = 1; a.A = A; a.Bc = Bc; a.G = G; }
    else { a.coef_eps = coef_eps; a.sigma = sigma; a.noise1 = noise1; }
    return dsh::launch_guided_ddim_step(a, ga, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_guided_ddpm_step(void* hip_stream, float* x, const float* eps, const float* noise, float* x0_out, const dsh_guide* guide, int32_t B,
                            int32_t frames, int32_t channels, float c1, float c2, float coef1, float coef2, float sigma, float post_var,
                            int32_t clip, int32_t c_lo, int32_t c_hi) {
    API_BEGIN
    DSH_REQUIRE(x && eps && noise && B > 0 && frames > 0 && channels > 0, "invalid argument");
    DSH_REQUIRE(c_lo >= 0 && c_hi <= channels, "guided_ddpm_step: channel range outside [0, channels]");
    dsh::GuideArgs ga;
    if (int e = guide_args("guided_ddpm_step", guide, B, frames, ga)) return e;
    ga.post_var = post_var;
    dsh::DdpmStepArgs a;
    a.x = x; a.eps = eps; a.noise = noise; a.x0_out = x0_out; a.c1 = c1; a.c2 = c2; a.coef1 = coef1; a.coef2 = coef2; a.sigma = sigma;
    a.clip = clip; a.n = (size_t)B * frames * channels; a.channels = channels; a.c_lo = c_lo; a.c_hi = c_hi;
    return dsh::launch_guided_ddpm_step(a, frames, ga, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_undo_step(void* hip_stream, float* x, const float* noise, float sqrt_1m_beta, float sqrt_beta, int64_t n, int32_t channels,
                     int32_t c_lo, int32_t c_hi) {
    API_BEGIN
    DSH_REQUIRE(x && noise && n >= 0, "invalid argument");
    return dsh::launch_undo_step(x, noise, sqrt_1m_beta, sqrt_beta, (size_t)n, reinterpret_cast<hipStream_t>(hip_stream), channels, c_lo, c_hi);
    API_END
}

int dsh_op_level_copy(void* hip_stream, void* const* work_dev, const int64_t* bytes, const int64_t* off, int32_t nseg, void* slots, int64_t stride,
                      const int64_t* level_dev, int32_t restore) {
    API_BEGIN
    DSH_REQUIRE(nseg >= 0 && nseg <= 4 && (nseg == 0 || (work_dev && bytes && off)) && slots && level_dev && stride >= 0, "level_copy: invalid argument");
    dsh::LevelCopyArgs a{};
    for (int i = 0; i < nseg; ++i) {
        DSH_REQUIRE(bytes[i] >= 0 && off[i] >= 0 && off[i] + bytes[i] <= stride && (bytes[i] == 0 || work_dev[i]), "level_copy: a range outside its slot");
        a.work[i] = reinterpret_cast<char*>(work_dev[i]); a.bytes[i] = (size_t)bytes[i]; a.off[i] = (size_t)off[i];
    }
    a.nseg = nseg; a.slots = reinterpret_cast<char*>(slots); a.stride = (size_t)stride; a.level = level_dev; a.restore = restore;
    return dsh::launch_level_copy(a, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_fill_step(void* hip_stream, int64_t* t, float* c1, float* c2, int64_t* level, int64_t tv, float c1v, float c2v, int64_t lv, int32_t n) {
    API_BEGIN
    DSH_REQUIRE(t && c1 && c2 && level && n > 0, "fill_step: invalid argument");
    return dsh::launch_fill_step(t, c1, c2, level, tv, c1v, c2v, lv, n, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_store_values_f32(void* hip_stream, float* p, const float* host, int32_t n) {
    API_BEGIN
    DSH_REQUIRE(p && host && n >= 0, "store_values_f32: invalid argument");
    return dsh::launch_store_values_f32(p, host, n, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_zero_padded_frames(void* hip_stream, float* x, const int32_t* lens_dev, int32_t B, int32_t frames, int32_t channels) {
    API_BEGIN
    return dsh::launch_zero_padded_frames(x, lens_dev, B, frames, channels, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_fill_cols(void* hip_stream, float* dst, int32_t C, int64_t M, int32_t c_lo, int32_t c_hi, const float* src, int32_t src_ld) {
    API_BEGIN
    return dsh::launch_fill_cols(dst, C, (size_t)M, c_lo, c_hi, src, src_ld, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_temb(void* hip_stream, int32_t dtype, const int64_t* t_dev, int32_t B, int32_t dim, void* out, int32_t ldo) {
    API_BEGIN
    DSH_REQUIRE(t_dev && out && B > 0 && dim >= 2 && dim % 2 == 0 && ldo >= dim && (dtype == 0 || dtype == 1), "temb: invalid argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    if (dtype == 0) return dsh::launch_temb_rows<float>(t_dev, B, dim, reinterpret_cast<float*>(out), ldo, s);
    return dsh::launch_temb_rows<dsh::bf16>(t_dev, B, dim, reinterpret_cast<dsh::bf16*>(out), ldo, s);
    API_END
}

int dsh_op_cfg_mix(void* hip_stream, const float* o, int32_t ldo, int32_t Mc, int32_t cond_row0, int32_t frames, int32_t w, int32_t has_null,
                   const float* scale, int32_t scale_row, float* eps, int32_t lde, int32_t c0, const float* x, int32_t ldx, const float* c1,
                   const float* c2, float* x0, int32_t ldx0) {
    API_BEGIN
    DSH_REQUIRE(o && eps && Mc > 0 && frames > 0 && w > 0 && ldo >= w && c0 >= 0 && lde >= c0 + w, "cfg_mix: invalid argument");
    DSH_REQUIRE(!has_null || cond_row0 >= Mc, "cfg_mix: the conditional half starts behind the unconditional one");
    DSH_REQUIRE(!x0 || (x && c1 && c2 && ldx >= c0 + w && ldx0 >= w), "cfg_mix: the x0 branch needs x, c1 and c2");
    return dsh::launch_cfg_mix(o, ldo, Mc, cond_row0, frames, w, has_null, scale, scale_row, eps, lde, c0, x, ldx, c1, c2, x0, ldx0,
                               reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_cfg_mix_sched(void* hip_stream, const float* o, int32_t ldo, int32_t Mc, int32_t cond_row0, int32_t frames, int32_t w, int32_t has_null,
                         const float* scale, int32_t scale_row, float* eps, int32_t lde, int32_t c0, const float* x, int32_t ldx, const float* c1,
                         const float* c2, float* x0, int32_t ldx0, const int64_t* t, int32_t t_row, const float* table, int32_t n_steps,
                         int32_t which, float rescale, const int32_t* lens_dev) {
    API_BEGIN
    DSH_REQUIRE(o && eps && Mc > 0 && frames > 0 && Mc % frames == 0 && w > 0 && ldo >= w && c0 >= 0 && lde >= c0 + w, "cfg_mix_sched: invalid argument");
    DSH_REQUIRE(!has_null || cond_row0 >= Mc, "cfg_mix_sched: the conditional half starts behind the unconditional one");
    DSH_REQUIRE(!x0 || (x && c1 && c2 && ldx >= c0 + w && ldx0 >= w), "cfg_mix_sched: the x0 branch needs x, c1 and c2");
    DSH_REQUIRE(rescale >= 0.0f && rescale <= 1.0f && (which == 0 || which == 1) && (t_row == 0 || t_row == 1) && (scale_row == 0 || scale_row == 1),
                "cfg_mix_sched: rescale in [0, 1], row 0 or 1, strides 0 or 1");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    // an undoubled batch has nothing to weigh: the schedule is inert, the plain launch
    if (!has_null) return dsh::launch_cfg_mix(o, ldo, Mc, cond_row0, frames, w, 0, scale, scale_row, eps, lde, c0, x, ldx, c1, c2, x0, ldx0, s);
    DSH_REQUIRE(scale && t && table && n_steps > 0, "cfg_mix_sched: a doubled batch needs scales, timesteps and the gain table");
    // the device table as the context keeps it: the two gain rows, then the two rescale factors (`rescale` is row `which`'s)
    OpScratch scratch;
    void *tab = nullptr, *part = nullptr;
    if (int e = scratch.alloc(&tab, ((size_t)2 * n_steps + 2) * sizeof(float))) return e;
    DSH_HIP_CHECK(hipMemcpyAsync(tab, table, (size_t)2 * n_steps * sizeof(float), hipMemcpyDeviceToDevice, s));
    const float phi[2] = {rescale, rescale};
    if (int e = dsh::launch_store_values_f32(reinterpret_cast<float*>(tab) + (size_t)2 * n_steps, phi, 2, s)) return e;
    if (rescale > 0.0f) { if (int e = scratch.alloc(&part, (size_t)Mc * 4 * sizeof(double))) return e; }
    const int rc = dsh::launch_cfg_mix_sched(o, ldo, Mc, cond_row0, frames, w, scale, scale_row, t, t_row, reinterpret_cast<const float*>(tab), n_steps,
                                             which, rescale > 0.0f, lens_dev, reinterpret_cast<double*>(part), eps, lde, c0, x, ldx, c1, c2, x0, ldx0, s);
    DSH_HIP_CHECK(hipStreamSynchronize(s));
    return rc;
    API_END
}

int dsh_op_im2col3(void* hip_stream, int32_t dtype_in, int32_t dtype_out, const void* x, int32_t ldx, int32_t B, int32_t frames, int32_t Cin,
                   void* out, int32_t ldo, const int32_t* lens_dev) {
    API_BEGIN
    DSH_REQUIRE(x && out && B > 0 && frames > 0 && Cin > 0 && ldx >= Cin && ldo >= 3 * Cin, "im2col3: invalid argument");
    DSH_REQUIRE((dtype_in == 0 || dtype_in == 1) && (dtype_out == 0 || dtype_out == 1) && !(dtype_in == 1 && dtype_out == 0),
                "im2col3: fp32 -> fp32, fp32 -> bf16 or bf16 -> bf16");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    if (dtype_in == 0 && dtype_out == 0)
        return dsh::launch_im2col3_rows<float, float>(reinterpret_cast<const float*>(x), ldx, B, frames, Cin, reinterpret_cast<float*>(out), ldo, s, lens_dev);
    if (dtype_in == 0)
        return dsh::launch_im2col3_rows<float, dsh::bf16>(reinterpret_cast<const float*>(x), ldx, B, frames, Cin, reinterpret_cast<dsh::bf16*>(out), ldo, s, lens_dev);
    return dsh::launch_im2col3_rows<dsh::bf16, dsh::bf16>(reinterpret_cast<const dsh::bf16*>(x), ldx, B, frames, Cin, reinterpret_cast<dsh::bf16*>(out), ldo, s, lens_dev);
    API_END
}

int dsh_op_film_fold(void* hip_stream, float* tab, int32_t ld, int32_t B, int32_t nblk, int32_t D, const float* gamma, const float* beta) {
    API_BEGIN
    DSH_REQUIRE(tab && gamma && beta && B > 0 && nblk > 0 && D > 0 && (int64_t)ld >= 2 * (int64_t)D * nblk, "film_fold: invalid argument");
    return dsh::launch_film_fold(tab, ld, B, nblk, D, gamma, beta, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_film_expand(void* hip_stream, const float* src, int32_t ld, const int32_t* idx_dev, float* dst, int32_t B, int32_t nblk, int32_t D,
                       const float* gamma, const float* beta, int32_t fold) {
    API_BEGIN
    DSH_REQUIRE(src && dst && B > 0 && nblk > 0 && D > 0 && (int64_t)ld >= 2 * (int64_t)D * nblk && (!fold || (gamma && beta)), "film_expand: invalid argument");
    return dsh::launch_film_expand(src, ld, idx_dev, dst, B, nblk, D, gamma, beta, fold, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_gather_rows(void* hip_stream, const float* src, int32_t ld, const int32_t* idx_dev, float* dst, int32_t ldd, int32_t B, int32_t w) {
    API_BEGIN
    DSH_REQUIRE(src && idx_dev && dst && B > 0 && w > 0 && ld >= w && ldd >= w, "gather_rows: invalid argument");
    return dsh::launch_gather_rows_f32(src, ld, idx_dev, dst, ldd, B, w, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_seed_stream(void* hip_stream, const float* h0, int32_t Mc, int32_t D, const float* c, int32_t has_null, int32_t row1, int32_t hilo,
                       float* h_out, void* h16_out, void* lo_out) {
    API_BEGIN
    DSH_REQUIRE(h0 && h16_out && Mc > 0 && D > 0 && D % 32 == 0 && (hilo ? lo_out != nullptr : h_out != nullptr), "seed_stream: null operand or output");
    DSH_REQUIRE(!has_null || row1 >= 0, "seed_stream: negative row1");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    OpScratch scratch;
    // tiled planes: the null half's blocks at row 0, the conditional half's at row1 — rows the kernel does not write come back as 0
    const int rows = (has_null ? row1 : 0) + dsh::round_up(Mc, 32);
    void *h = nullptr, *h16 = nullptr, *lo = nullptr;
    if (int e = scratch.alloc(&h16, (size_t)rows * D * 2)) return e;
    DSH_HIP_CHECK(hipMemsetAsync(h16, 0, (size_t)rows * D * 2, s));
    if (hilo) {
        if (int e = scratch.alloc(&lo, (size_t)rows * D * 2)) return e;
        DSH_HIP_CHECK(hipMemsetAsync(lo, 0, (size_t)rows * D * 2, s));
    } else {
        if (int e = scratch.alloc(&h, (size_t)rows * D * 4)) return e;
        DSH_HIP_CHECK(hipMemsetAsync(h, 0, (size_t)rows * D * 4, s));
    }
    int rc = dsh::launch_seed_stream(h0, Mc, D, c, has_null, row1, reinterpret_cast<float*>(h), h16, s, lo);
    if (!rc && h) rc = dsh::launch_untile_rows_f32(reinterpret_cast<const float*>(h), D, rows, h_out, D, s);
    if (!rc) rc = dsh::launch_untile_rows_bf16(h16, D, rows, D, h16_out, D, s);
    if (!rc && lo) rc = dsh::launch_untile_rows_bf16(lo, D, rows, D, lo_out, D, s);
    DSH_HIP_CHECK(hipStreamSynchronize(s));
    return rc;
    API_END
}

int dsh_op_pack_expr_track(void* hip_stream, const float* src, int32_t E, int32_t B, int32_t frames, const int32_t* lens_dev, float* x0, int32_t ld,
                           void* x16_out, void* tiler_out) {
    API_BEGIN
    DSH_REQUIRE(src && x0 && B > 0 && frames > 0, "pack_expr_track: invalid argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    OpScratch scratch;
    const int M = B * frames, Mp = dsh::round_up(M, 32);
    void *x16 = nullptr, *tl = nullptr;
    if (x16_out) { if (int e = scratch.alloc(&x16, (size_t)Mp * 128 * 2)) return e; }
    int rc = dsh::launch_pack_expr_track(src, E, B, frames, lens_dev, x0, ld, x16, s);
    if (!rc && x16) rc = dsh::launch_untile_rows_bf16(x16, 128, M, 128, x16_out, 128, s);
    if (!rc && tiler_out) {            // the production tiler on the x0 rows just written: what the header promises x16 to equal
        if (int e = scratch.alloc(&tl, (size_t)Mp * 128 * 2)) return e;
        rc = dsh::launch_tile_rows_bf16<float>(x0, ld, M, ld, tl, 128, s);
        if (!rc) rc = dsh::launch_untile_rows_bf16(tl, 128, M, 128, tiler_out, 128, s);
    }
    DSH_HIP_CHECK(hipStreamSynchronize(s));
    return rc;
    API_END
}

int dsh_op_layernorm_pre(void* hip_stream, int32_t dtype, float* h, int32_t ldh, int32_t M, int32_t D, const float* pre_add, int32_t n_pre_rows,
                         const float* gamma, const float* beta, void* out, int32_t ldo) {
    API_BEGIN
    DSH_REQUIRE(h && gamma && beta && out && M > 0 && D > 0 && ldh >= D && ldo >= D && (dtype == 0 || dtype == 1), "layernorm_pre: invalid argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    if (dtype == 0) return dsh::launch_ln_rows<float>(h, ldh, M, D, pre_add, n_pre_rows, gamma, beta, reinterpret_cast<float*>(out), ldo, s);
    return dsh::launch_ln_rows<dsh::bf16>(h, ldh, M, D, pre_add, n_pre_rows, gamma, beta, reinterpret_cast<dsh::bf16*>(out), ldo, s);
    API_END
}

int dsh_op_ln_film_silu(void* hip_stream, int32_t variant, const void* y, int32_t ldy, int32_t M, int32_t D, const float* gamma, const float* beta,
                        const float* film, int32_t film_ld, int32_t film_off, int32_t frames, int32_t bmod, void* out, int32_t ldo) {
    API_BEGIN
    DSH_REQUIRE(y && gamma && beta && film && out && M > 0 && D > 0 && ldy >= D && ldo >= D && frames > 0 && bmod > 0 && film_off >= 0 &&
                film_ld >= film_off + 2 * D && variant >= 0 && variant <= 2, "ln_film_silu: invalid argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    if (variant == 0)
        return dsh::launch_ln_film_silu_rows<float, float>(reinterpret_cast<const float*>(y), ldy, M, D, gamma, beta, film, film_ld, film_off, frames, bmod,
                                                           reinterpret_cast<float*>(out), ldo, s);
    if (variant == 1)
        return dsh::launch_ln_film_silu_rows<float, dsh::bf16>(reinterpret_cast<const float*>(y), ldy, M, D, gamma, beta, film, film_ld, film_off, frames, bmod,
                                                               reinterpret_cast<dsh::bf16*>(out), ldo, s);
    return dsh::launch_ln_film_silu_rows<dsh::bf16, dsh::bf16>(reinterpret_cast<const dsh::bf16*>(y), ldy, M, D, gamma, beta, film, film_ld, film_off, frames,
                                                               bmod, reinterpret_cast<dsh::bf16*>(out), ldo, s);
    API_END
}

int dsh_op_concat_ln(void* hip_stream, int32_t dtype, const float* p0, int32_t ld0, int32_t w0, const void* p1, int32_t ld1, int32_t w1,
                     const void* p2, int32_t ld2, int32_t w2, const float* p3, int32_t ld3, int32_t w3, int32_t M, const float* gamma,
                     const float* beta, void* out, int32_t ldo, int32_t Ppad) {
    API_BEGIN
    DSH_REQUIRE(p0 && p1 && p2 && (w3 == 0 || p3) && gamma && beta && out && M > 0 && (dtype == 0 || dtype == 1), "concat_ln: invalid argument");
    DSH_REQUIRE(w0 > 0 && w1 > 0 && w2 > 0 && w3 >= 0 && ld0 >= w0 && ld1 >= w1 && ld2 >= w2 && ld3 >= w3 && Ppad >= w0 + w1 + w2 + w3 && ldo >= Ppad,
                "concat_ln: segment widths, leading dimensions and the padded width");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    dsh::ConcatSegs sg{p0, ld0, w0, p1, ld1, w1, p2, ld2, w2, p3, ld3, w3};
    if (dtype == 0) return dsh::launch_concat_ln_rows<float>(sg, M, gamma, beta, reinterpret_cast<float*>(out), ldo, Ppad, s);
    return dsh::launch_concat_ln_rows<dsh::bf16>(sg, M, gamma, beta, reinterpret_cast<dsh::bf16*>(out), ldo, Ppad, s);
    API_END
}

// ---- validation metrics: FGD pose encoder + per-batch metrics (pose_encoder.hip, metrics.hip) ----------------------
struct dsh_fgd {
    std::unique_ptr<dsh::FgdEncoder> enc;
};

int dsh_fgd_create(int32_t n_poses, int32_t dim, int32_t vae_length, void* hip_stream, dsh_fgd** out) {
    API_BEGIN
    DSH_REQUIRE(out, "null argument");
    DSH_REQUIRE(dim > 0 && vae_length > 0 && vae_length % 4 == 0, "dsh_fgd_create: dim must be positive and vae_length a positive multiple of 4");
    DSH_REQUIRE(n_poses >= 12, "dsh_fgd_create: n_poses too small for the four convolutions (kernel 3, 3, 4 / stride 2, 3)");
    auto h = std::make_unique<dsh_fgd>();
    h->enc.reset(new dsh::FgdEncoder(n_poses, dim, vae_length, reinterpret_cast<hipStream_t>(hip_stream)));
    *out = h.release();
    return 0;
    API_END
}

int dsh_fgd_destroy(dsh_fgd* h) {
    API_BEGIN
    delete h;
    return 0;
    API_END
}

int32_t dsh_fgd_debug_num_layers(const dsh_fgd* h) { return h ? h->enc->num_layers() : -1; }

int dsh_fgd_debug_packed_layer(const dsh_fgd* h, int32_t index, int32_t* dims3, float* W, float* bias) {
    API_BEGIN
    DSH_REQUIRE(h, "null handle");
    return h->enc->packed_layer(index, dims3, W, bias);
    API_END
}

int dsh_fgd_load_tensor(dsh_fgd* h, const char* name, const float* host_data, const int64_t* shape, int32_t ndim) {
    API_BEGIN
    DSH_REQUIRE(h && name && (shape || ndim == 0) && ndim >= 0, "null argument");
    return h->enc->load(name, host_data, shape, ndim);
    API_END
}

int dsh_fgd_finalize(dsh_fgd* h) {
    API_BEGIN
    DSH_REQUIRE(h, "null handle");
    return h->enc->finalize();
    API_END
}

int dsh_fgd_encode(dsh_fgd* h, const float* x, int32_t batch, int32_t frames, float* latents) {
    API_BEGIN
    DSH_REQUIRE(h, "null handle");
    return h->enc->encode(x, batch, frames, latents);
    API_END
}

int dsh_op_conv_gemm_f32(void* hip_stream, const float* X, int64_t x_clip, int32_t x_step, const float* W, int32_t ldw, const float* bias, float* Y,
                         int64_t y_clip, int32_t B, int32_t Tout, int32_t N, int32_t Kreal, int32_t Kp, int32_t leaky) {
    API_BEGIN
    DSH_REQUIRE(X && W && bias && Y, "dsh_op_conv_gemm_f32: null pointer");
    DSH_REQUIRE(B > 0, "dsh_op_conv_gemm_f32: B must be positive");
    DSH_REQUIRE(Tout <= 0 || (long long)B * Tout < (1ll << 31), "dsh_op_conv_gemm_f32: B * Tout must fit an int");
    dsh::ConvGemmArgs a{};
    a.X = X; a.x_clip = x_clip; a.x_step = x_step;
    a.W = W; a.ldw = ldw; a.bias = bias;
    a.Y = Y; a.y_clip = y_clip;
    a.Tout = Tout; a.M = Tout > 0 ? B * Tout : 0; a.N = N; a.Kreal = Kreal; a.Kp = Kp;
    a.leaky = leaky ? 1 : 0;
    return dsh::launch_conv_gemm_f32(a, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int64_t dsh_batch_metrics_result_bytes(int32_t B, int32_t T, int32_t C, int32_t b_div) { return dsh::batch_metrics_result_bytes(B, T, C, b_div); }

int dsh_op_batch_metrics(void* hip_stream, const float* outputs, const float* motions, int32_t B, int32_t T, int32_t C, int32_t joint_dim,
                         int32_t b_div, void* result_dev) {
    API_BEGIN
    return dsh::launch_batch_metrics(outputs, motions, B, T, C, joint_dim, b_div, result_dev, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int64_t dsh_denoise_losses_result_bytes(int32_t B, int32_t T) { return dsh::denoise_losses_result_bytes(B, T); }

int dsh_op_denoise_losses(void* hip_stream, const float* eps, const float* noise, const float* x_t, const float* x0, const float* c1_dev,
                          const float* c2_dev, const int32_t* lens_dev, int32_t B, int32_t T, int32_t C, int32_t split, float huber_beta,
                          float* x0_pred_out, float* frame_mse_out, void* result_dev) {
    API_BEGIN
    return dsh::launch_denoise_losses(eps, noise, x_t, x0, c1_dev, c2_dev, lens_dev, B, T, C, split, huber_beta, x0_pred_out, frame_mse_out,
                                      result_dev, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

// ---- audio front: mel spectrogram, polyphase resampler, softmax attention core (audio_front.hip) ----------------------
struct dsh_mel {
    std::unique_ptr<dsh::MelFront> m;
};

int dsh_mel_create(int32_t sr, int32_t n_fft, int32_t hop, int32_t n_mels, void* hip_stream, dsh_mel** out) {
    API_BEGIN
    DSH_REQUIRE(out, "null argument");
    DSH_REQUIRE(sr > 0 && n_fft >= 32 && n_fft % 32 == 0 && n_fft <= 16384, "dsh_mel_create: n_fft must be a multiple of 32, at most 16384");
    DSH_REQUIRE(hop >= 4 && hop % 4 == 0, "dsh_mel_create: hop must be a positive multiple of 4 (16-byte frame starts)");
    DSH_REQUIRE(n_mels >= 4 && n_mels % 4 == 0 && n_mels <= 1024, "dsh_mel_create: n_mels must be a multiple of 4, at most 1024");
    auto h = std::make_unique<dsh_mel>();
    h->m.reset(new dsh::MelFront(sr, n_fft, hop, n_mels, reinterpret_cast<hipStream_t>(hip_stream)));
    *out = h.release();
    return 0;
    API_END
}

int dsh_mel_destroy(dsh_mel* h) {
    API_BEGIN
    delete h;
    return 0;
    API_END
}

int64_t dsh_mel_num_frames(const dsh_mel* h, int64_t len) { return h ? h->m->num_frames(len) : -1; }

int dsh_mel_debug_tables(const dsh_mel* h, int32_t* dims3, float* dft, float* fb) {
    API_BEGIN
    DSH_REQUIRE(h, "null handle");
    if (dims3) { dims3[0] = h->m->bins(); dims3[1] = h->m->n_fft(); dims3[2] = h->m->n_mels(); }
    if (dft) memcpy(dft, h->m->dft().data(), h->m->dft().size() * sizeof(float));
    if (fb) memcpy(fb, h->m->fb().data(), h->m->fb().size() * sizeof(float));
    return 0;
    API_END
}

int dsh_mel_compute(dsh_mel* h, const float* wave, int32_t batch, int64_t len, float* mel) {
    API_BEGIN
    DSH_REQUIRE(h, "null handle");
    return h->m->compute(wave, batch, len, mel);
    API_END
}

int dsh_mel_compute_ragged(dsh_mel* h, const float* wave, int32_t batch, int64_t len, const int32_t* lens_dev, float* mel) {
    API_BEGIN
    DSH_REQUIRE(h, "null handle");
    return h->m->compute_ragged(wave, batch, len, lens_dev, mel);
    API_END
}

int64_t dsh_resample_poly_len(int64_t n, int32_t up, int32_t down) { return n >= 0 && up > 0 && down > 0 ? dsh::resample_poly_len(n, up, down) : -1; }

int dsh_op_resample_poly(void* hip_stream, const float* x, int32_t batch, int64_t n, int32_t up, int32_t down, const float* taps_dev, int32_t n_taps,
                         float* y) {
    API_BEGIN
    return dsh::launch_resample_poly(x, batch, n, up, down, taps_dev, n_taps, y, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_resample_poly_ragged(void* hip_stream, const float* x, int32_t batch, int64_t n, const int32_t* lens_dev, int32_t up, int32_t down,
                                const float* taps_dev, int32_t n_taps, float* y) {
    API_BEGIN
    DSH_REQUIRE(lens_dev, "dsh_op_resample_poly_ragged: null lengths");
    return dsh::launch_resample_poly_ragged(x, batch, n, lens_dev, up, down, taps_dev, n_taps, y, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_softmax_attention_ragged(void* hip_stream, const float* qkv, int32_t B, int32_t M_max, int32_t H, const int32_t* lens_dev, float* out) {
    API_BEGIN
    return dsh::launch_softmax_attention_ragged(qkv, B, M_max, H, lens_dev, out, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_softmax_attention(void* hip_stream, const float* qkv, int32_t B, int32_t M, int32_t H, float* out) {
    API_BEGIN
    return dsh::launch_softmax_attention(qkv, B, M, H, out, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

// ---- HuBERT encoder (hubert.hip) ----------------------------------------------------------------------------------------
struct dsh_hubert {
    std::unique_ptr<dsh::HubertEncoder> enc;
};

int dsh_hubert_create(const dsh_hubert_config* cfg, void* hip_stream, dsh_hubert** out) {
    API_BEGIN
    DSH_REQUIRE(cfg && out, "null argument");
    dsh::HubertConfig c{};
    c.hidden = cfg->hidden; c.layers = cfg->layers; c.heads = cfg->heads; c.intermediate = cfg->intermediate;
    for (int i = 0; i < 7; ++i) { c.conv_dim[i] = cfg->conv_dim[i]; c.conv_kernel[i] = cfg->conv_kernel[i]; c.conv_stride[i] = cfg->conv_stride[i]; }
    c.pos_kernel = cfg->pos_kernel; c.pos_groups = cfg->pos_groups; c.ln_eps = cfg->ln_eps;
    if (int e = dsh::HubertEncoder::validate(c)) return e;
    auto h = std::make_unique<dsh_hubert>();
    h->enc.reset(new dsh::HubertEncoder(c, reinterpret_cast<hipStream_t>(hip_stream)));
    *out = h.release();
    return 0;
    API_END
}

int dsh_hubert_destroy(dsh_hubert* h) {
    API_BEGIN
    delete h;
    return 0;
    API_END
}

int dsh_hubert_load_tensor(dsh_hubert* h, const char* name, const float* host_data, const int64_t* shape, int32_t ndim) {
    API_BEGIN
    DSH_REQUIRE(h && name && (shape || ndim == 0) && ndim >= 0, "null argument");
    return h->enc->load(name, host_data, shape, ndim);
    API_END
}

int dsh_hubert_finalize(dsh_hubert* h) {
    API_BEGIN
    DSH_REQUIRE(h, "null handle");
    return h->enc->finalize();
    API_END
}

int dsh_hubert_debug_packed(const dsh_hubert* h, int32_t kind, int32_t layer, int32_t* dims2, float* W, float* bias, float* fc) {
    API_BEGIN
    DSH_REQUIRE(h, "null handle");
    return h->enc->debug_packed(kind, layer, dims2, W, bias, fc);
    API_END
}

int64_t dsh_hubert_num_frames(const dsh_hubert* h, int64_t n) { return h ? h->enc->num_frames(n) : -1; }

int dsh_hubert_set_precision(dsh_hubert* h, int32_t precision) {
    API_BEGIN
    DSH_REQUIRE(h, "null handle");
    return h->enc->set_precision(precision);
    API_END
}

int dsh_hubert_debug_tap(dsh_hubert* h, float* h_posconv_dev) {
    API_BEGIN
    DSH_REQUIRE(h, "null handle");
    h->enc->set_debug_tap(h_posconv_dev);
    return 0;
    API_END
}

int dsh_op_gemm_bf16_pro(void* hip_stream, const void* A, int32_t a_f32, const float* mom, const void* W, const float* bias, const float* R,
                         float* Cf, void* Cb, int32_t M, int32_t N, int32_t K, int32_t act, int32_t tile) {
    API_BEGIN
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    DSH_REQUIRE(A && M >= 1 && K >= 64 && K % 64 == 0, "dsh_op_gemm_bf16_pro: M >= 1, K a multiple of 64");
    OpScratch scratch;
    dsh::GemmBf16ProArgs a{};
    a.A = A; a.lda = K; a.a_f32 = a_f32 ? 1 : 0; a.mom = mom;
    if (a_f32 && !mom) {                       // the rows' own two-pass moments (eps 1e-5), as the encoder launches them in front of the Linear
        DSH_REQUIRE(K <= 1024, "dsh_op_gemm_bf16_pro: LayerNorm rows of at most 1024 channels");
        void* m = nullptr;
        if (int e = scratch.alloc(&m, (size_t)M * 2 * sizeof(float))) return e;
        if (int e = dsh::launch_row_moments(static_cast<const float*>(A), M, K, 1e-5f, static_cast<float*>(m), s)) return e;
        a.mom = static_cast<const float*>(m);
    }
    // W arrives in natural [N, K] order, which is the kernel's packed order (gemm_bf16_pro.hip): nothing to permute
    a.W = static_cast<const dsh::bf16*>(W); a.bias = bias; a.R = R; a.Cf = Cf; a.Cb = static_cast<dsh::bf16*>(Cb);
    a.M = M; a.N = N; a.K = K; a.act = act; a.tile = tile;
    if (int e = dsh::launch_gemm_bf16_pro(a, s)) return e;
    if (!scratch.p.empty()) DSH_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
    API_END
}

int dsh_op_softmax_attention_bf16(void* hip_stream, const void* qkv, int32_t B, int32_t M, int32_t H, void* out) {
    API_BEGIN
    return dsh::launch_softmax_attention_bf16(static_cast<const dsh::bf16*>(qkv), B, M, H, static_cast<dsh::bf16*>(out), reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_softmax_attention_bf16_ragged(void* hip_stream, const void* qkv, int32_t B, int32_t M_max, int32_t H, const int32_t* lens_dev, void* out) {
    API_BEGIN
    return dsh::launch_softmax_attention_bf16_ragged(static_cast<const dsh::bf16*>(qkv), B, M_max, H, lens_dev, static_cast<dsh::bf16*>(out),
                                                     reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_hubert_set_chunk_pass(dsh_hubert* h, int32_t rows) {
    API_BEGIN
    DSH_REQUIRE(h && rows >= 1, "dsh_hubert_set_chunk_pass: a handle and at least one row per pass");
    h->enc->set_chunk_pass(rows);
    return 0;
    API_END
}

int dsh_hubert_encode(dsh_hubert* h, const float* x, int32_t batch, int64_t n, float* out) {
    API_BEGIN
    DSH_REQUIRE(h, "null handle");
    return h->enc->encode(x, batch, n, out);
    API_END
}

int dsh_hubert_encode_ragged(dsh_hubert* h, const float* x, int32_t batch, int64_t n_max, const int64_t* lens_samples, float* out) {
    API_BEGIN
    DSH_REQUIRE(h, "null handle");
    return h->enc->encode_ragged(x, batch, n_max, lens_samples, out);
    API_END
}

int dsh_op_pos_conv_ragged(void* hip_stream, const float* h, int32_t B, int32_t M_max, int32_t hidden, int32_t groups, int32_t pos_kernel,
                           const float* W, const float* bias, const int32_t* lens_dev, float* out) {
    API_BEGIN
    DSH_REQUIRE(lens_dev, "dsh_op_pos_conv_ragged: null lengths");
    return dsh::launch_pos_conv(h, B, M_max, hidden, groups, pos_kernel, W, bias, out, reinterpret_cast<hipStream_t>(hip_stream), lens_dev);
    API_END
}

int dsh_op_pos_conv(void* hip_stream, const float* h, int32_t B, int32_t M, int32_t hidden, int32_t groups, int32_t pos_kernel, const float* W,
                    const float* bias, float* out) {
    API_BEGIN
    return dsh::launch_pos_conv(h, B, M, hidden, groups, pos_kernel, W, bias, out, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_conv0_ln_gelu(void* hip_stream, const float* x, int32_t B, int64_t n, int32_t C, int32_t k, int32_t stride, const float* W, const float* bias,
                         const float* gamma, const float* beta, float* y) {
    API_BEGIN
    DSH_REQUIRE(k >= 1 && stride >= 1 && n >= k, "dsh_op_conv0_ln_gelu: the signal is shorter than the kernel");
    return dsh::launch_conv0_ln_gelu(x, B, n, (int)((n - k) / stride + 1), C, k, stride, W, bias, gamma, beta, y, reinterpret_cast<hipStream_t>(hip_stream));
    API_END
}

int dsh_op_conv_ln_gelu(void* hip_stream, const float* x, int32_t B, int32_t L, int32_t Cin, int32_t Cout, int32_t k, int32_t stride, const float* W,
                        const float* bias, const float* gamma, const float* beta, float* y) {
    API_BEGIN
    DSH_REQUIRE(x && W && bias && gamma && beta && y, "dsh_op_conv_ln_gelu: null pointer");
    DSH_REQUIRE(B >= 1 && k >= 1 && stride >= 1 && L >= k && Cin % 32 == 0 && Cout % 32 == 0 && Cin > 0 && Cout > 0,
                "dsh_op_conv_ln_gelu: channel counts must be multiples of 32 and the clip at least one kernel long");
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    const int Lo = (L - k) / stride + 1;
    DSH_REQUIRE((long long)B * Lo < (1ll << 31), "dsh_op_conv_ln_gelu: batch too large");
    dsh::ConvGemmArgs a{};
    a.X = x; a.x_clip = (long long)L * Cin; a.x_step = stride * Cin;
    a.W = W; a.ldw = k * Cin; a.bias = bias;
    a.Y = y; a.y_clip = (long long)Lo * Cout;
    a.Tout = Lo; a.M = B * Lo; a.N = Cout; a.Kreal = k * Cin; a.Kp = k * Cin;
    if (int e = dsh::launch_conv_gemm_f32(a, s)) return e;
    return dsh::launch_ln_act_rows(y, (long long)B * Lo, Cout, gamma, beta, 1e-5f, 1, y, s);
    API_END
}

}  // extern "C"
