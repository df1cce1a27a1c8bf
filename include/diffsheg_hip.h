/*
 * diffsheg_hip.h — C ABI of the MI355X-native DiffSHEG sampling hot path (libdiffsheg_hip.so).
 *
 * The reference is pure Python/PyTorch; it has no FFI for this path.  The entry points below are
 * what a binding for the three in-process boundaries of the reference would call:
 *
 *   boundary 1  model(x, ts, **model_kwargs)          models/gaussian_diffusion.py:536
 *               (through _WrappedModel.__call__,       models/respace.py:119-124;
 *                UniDiffuser.forward                   models/transformer.py:728-770)   -> dsh_eval
 *   boundary 2  ddim_sample_loop / p_sample_loop       models/gaussian_diffusion.py:1106-1159, :776-841
 *               (SpacedDiffusion tables                models/respace.py:68-82,
 *                jump schedule                         models/scheduler.py:178-208)     -> dsh_sample
 *   weights     UniDiffuser.state_dict() key names     trainers/ddpm_show_trainer.py:259-292 -> dsh_load_tensor
 *
 * Conventions: every pointer marked "device" is caller-owned HIP device memory on the context's
 * device; tensors are dense row-major float32 [B,T,channels] unless stated; timesteps are int64.
 * Functions return 0 on success, negative on error (-1 invalid argument, -2 HIP runtime error,
 * -3 a C++ exception such as std::bad_alloc caught at the boundary); dsh_last_error() returns a
 * thread-local description.  No exceptions cross this boundary.  A
 * context is bound to one (device, stream) and is not thread-safe; distinct contexts are
 * independent (one process per GPU, as runner.py:86 mp.spawn does).
 */
#ifndef DIFFSHEG_HIP_H
#define DIFFSHEG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dsh_ctx dsh_ctx;

/* DSH_PRECISION_BF16X3: the fp32 path (fp32 storage, row kernels, attention core, sampler) with its large Linears (gemm_f32_pro) formed as three
 * bf16 MFMAs per product on hi / lo bf16 pieces of both operands (gemm_f32_split.hip): ~2^-16 relative per product instead of fp32's 2^-24.  At or
 * below the few-row threshold (DSH_GEMM_KSPLIT, 512 token rows) it launches the very kernels of DSH_PRECISION_FP32 and is bit-identical to it. */
enum { DSH_PRECISION_FP32 = 0, DSH_PRECISION_BF16 = 1, DSH_PRECISION_BF16X3 = 2 };
enum { DSH_SAMPLER_DDIM = 0, DSH_SAMPLER_DDPM = 1 };
enum { DSH_NOISE_STACK = 0, DSH_NOISE_PHILOX = 1 };

/* Static model configuration: the attributes UniDiffuser reads off the reference's `opt`
 * namespace (runner.py:124-222, options/base_options.py), baked at creation. */
typedef struct dsh_model_config {
    int32_t dim_pose;        /* gesture channels (129 SHOW / 141 BEAT)   */
    int32_t expression_dim;  /* expression channels (103 / 51)           */
    int32_t style_dim;       /* one-hot speaker width (4 / 30)           */
    int32_t classifier_free; /* model has null_cond_emb                  */
    float   cond_scale;      /* initial CFG scale (dsh_set_guidance_scale) */
    int32_t latent_dim;      /* 512  */
    int32_t ff_size;         /* 1024 */
    int32_t num_layers;      /* 8    */
    int32_t num_heads;       /* 8    */
    int32_t audio_dim;       /* 128  */
    int32_t aud_latent_dim;  /* 256  */
    int32_t hubert_dim;      /* 1024 */
    int32_t hubert_enc_dim;  /* 128  */
    int32_t precision;       /* DSH_PRECISION_*                          */
    int32_t single_transformer; /* 0: UniDiffuser (encoder_aud + encoder_exp -> encoder_ges), state-dict keys as saved by  */
                             /* runner.py:32-45.  1: ONE MotionTransformer over all dim_pose + expression_dim channels     */
                             /* (runner.py:46-57, opt.unidiffuser = False, model_base 'transformer_encoder'): keys without */
                             /* the encoder_* prefix, audio_proj on the 128 mel features; c1 / c2 of dsh_eval are unused   */
    int32_t diffusion_steps; /* length of the original timestep scale (0: 1000): entries of a guidance schedule's gain rows       */
} dsh_model_config;

/* Sampler options = the `opt` attributes read by gaussian_diffusion.py / respace.py / scheduler.py. */
typedef struct dsh_sampler_opts {
    int32_t kind;            /* DSH_SAMPLER_DDIM (spaced) or DSH_SAMPLER_DDPM (ancestral)            */
    int32_t diffusion_steps; /* 1000                                                                  */
    int32_t respacing;       /* K of 'ddimK' (25); ignored for DDPM                                   */
    int32_t jump_length;     /* RePaint jump schedule (options/base_options.py:127-128)               */
    int32_t jump_n_sample;
    int32_t overlap_len;     /* frames cross-faded when add_blend (gaussian_diffusion.py:1051-1054)   */
    int32_t add_blend;
    int32_t no_resample;     /* jump schedule with jump_length = jump_n_sample = 1                    */
    int32_t no_repaint;      /* plain 25-step loop even when a mask is present                        */
    int32_t clip_denoised;   /* clamp pred_xstart to [-1,1] (gaussian_diffusion.py:575-580); harness: 0 */
    int32_t noise_mode;      /* DSH_NOISE_STACK: consume caller-provided draws in reference order;    */
                             /* DSH_NOISE_PHILOX: on-device Philox4x32-10 + Box-Muller                */
    uint64_t seed;           /* Philox key                                                            */
    int32_t same_overlap_noisy; /* --same_overlap_noisy (gaussian_diffusion.py:1040-1060): out-painted frames take the  */
                             /* previous window's noisy tail of the same level, saved in the context after every DDIM   */
                             /* step (the reference's self.saved_noisy_tail); DDIM only                                 */
    int32_t clip_idx;        /* window index inside the chain (model_kwargs['y']['clip_idx']); 0 = first window         */
    float eta;               /* DDIM eta (gaussian_diffusion.py:985,1011-1032); the harness uses 0                       */
} dsh_sampler_opts;

const char* dsh_last_error(void);
const char* dsh_version(void);

/* ---- runtime switches (the DSH_* environment variables; csrc/switches.h holds the one table) -- no GPU needed -------------------- */
/* dsh_switch_count(): entries of the table.
 * dsh_switch_info(i, ...): entry i — the variable's name, its default as text, when it is read (0 PROCESS: latched by the first read in
 *   the process; 1 CONTEXT: at dsh_create; 2 CALL: on every call that uses it), its class (0 product, 1 A/B with bit-identical arms,
 *   2 A/B with round-off between the arms, 3 bench only: results may be garbage) and one line of meaning; static strings, any output
 *   pointer may be null.  Returns the kind (0 integer, 1 present-or-absent, 2 string), -1 for an index outside the table.
 * dsh_switch_read(name, &is_set, &value): the switch as the library itself reads it now — the latched value of a PROCESS entry (this
 *   read latches it if nothing has yet), a fresh look otherwise; value = atoi of the text, the entry's default when unset.  `name`
 *   may also be one of the library's derivations over the switches (dual_streams, ffn_generation, ffn_pc, ffn_pb, hilo_denoiser,
 *   hilo_op, pipe_switches_on, ...: kSwitchDerived in switches.h): value = what the library derives, is_set = 0.  -1: unknown name. */
int32_t dsh_switch_count(void);
int dsh_switch_info(int32_t i, const char** name, const char** default_text, int32_t* when, int32_t* cls, const char** help);
int dsh_switch_read(const char* name, int32_t* is_set, int64_t* value);

/* ---- lifecycle ------------------------------------------------------------------------------ */
/* `hip_stream` is a hipStream_t (NULL = default stream) on the current device. */
int dsh_create(const dsh_model_config* cfg, void* hip_stream, dsh_ctx** out);
int dsh_destroy(dsh_ctx* ctx);

/* ---- weights (state-dict key names of UniDiffuser; fp32 host memory, copied) ---------------- */
int dsh_load_tensor(dsh_ctx* ctx, const char* name, const float* host_data, const int64_t* shape, int32_t ndim);
/* Builds the device-side layout (fused qkv, stacked FiLM, folded BatchNorm, K-padded tiles,
 * feat_proj(null_cond_emb) constants) and releases the host staging copies. */
int dsh_finalize_weights(dsh_ctx* ctx);
int64_t dsh_weight_bytes(const dsh_ctx* ctx);

/* ---- boundary 1: one denoiser evaluation ------------------------------------------------------ */
/* Step-invariant conditioning (model_kwargs audio_emb / person_id / add_cond['pretrain_aud_feat']):
 *   audio_emb [B,T,audio_dim], person_id [B,style_dim], hubert [B,T,hubert_dim]; all device fp32.
 * Runs hubert_encoder and pid_embed once; must be called before dsh_eval / dsh_sample and again
 * whenever the conditioning or (B,T) changes.  The three tensors are copied into context-owned
 * buffers in stream order: they may be freed / overwritten as soon as the call has returned,
 * provided that happens on (or is ordered after) the context stream.
 * Shape limit (bf16 precision only): windows of 10 frames or fewer are evaluated in batches of at most 6 clips.  The
 * StylizationBlock launches stage the FiLM rows of every clip a token block touches: at most 4 clips per 32-token block
 * (window-chain kernels) or 6 per 128-token block (first-generation kernels), so min(31 / T + 2, B) <= 4 or
 * min(127 / T + 2, B) <= 6 must hold (integer division) - true for every T >= 11 and for every B <= 6.  A batch outside that
 * (B >= 7 with T <= 10) is refused HERE with -1, before any state changes and before any launch: the previous condition stays
 * usable, and dsh_eval / dsh_sample never see such a shape.  Split such a batch of chain tail windows into calls of at most 6
 * clips, or use fp32, which has no such limit.  (With DSH_TLS=0 or DSH_HILO=0 only the 128-token rule applies: B >= 7 needs T >= 26.) */
int dsh_set_condition(dsh_ctx* ctx, int32_t batch, int32_t frames, const float* audio_emb, const float* person_id,
                      const float* hubert);
/* Clips of different lengths in one batch.  The tensors are padded to frames_pad frames per clip ([B,frames_pad,...], as above) and
 * lengths_host[b] (HOST int32, 1 .. frames_pad) is the number of valid frames of clip b.  Definition: frames [0, lengths[b]) of every
 * output of dsh_eval / dsh_sample equal what the same clip gives evaluated / sampled ALONE at T = lengths[b]; they never depend on what
 * the padded frames of any input hold (finite values).  Frames >= lengths[b] of dsh_sample's result are exactly 0 (rows of `trace` are
 * not zeroed); of dsh_eval's output they are unspecified, finite for finite inputs.  (The reference has no such mode: with length < T
 * it masks encoder_aud only, transformer.py:563, :744, and never calls itself that way.)
 * The lengths are part of the condition (hubert_encoder and encoder_aud's hoisted attention depend on them): they are copied into a
 * context-owned device buffer which the attention kernels and the two hubert_encoder convolutions read when they run.  Everything else in
 * the model is per token and runs on all B x frames_pad rows: the regime decisions (graphs / pipeline / sub-batch streams, kernel
 * families, the shape limit above) and dsh_eval_flops keep using B x frames_pad — padded rows are computed and discarded.
 * dsh_set_condition keeps its meaning (every clip full) and clears the lengths.
 * With dsh_sample_set_row_keys, row b advances its Philox stream by lengths[b] * channels / 4 counters per draw (its own size), so a clip
 * draws the same noise padded as alone; lengths[b] * channels % 4 == 0 is then required.  The whole-batch stream and noise stacks are
 * addressed by the padded shape as before.
 * -1 before any state changes (the previous condition stays usable) on a length < 1 or > frames_pad; dsh_sample returns -1 with lengths set
 * together with same_overlap_noisy or dsh_sample_set_tail_blend (both address the last overlap_len frames of the padded window). */
int dsh_set_condition_ragged(dsh_ctx* ctx, int32_t batch, int32_t frames_pad, const int32_t* lengths_host, const float* audio_emb,
                             const float* person_id, const float* hubert);
/* One modality alone.  modality: 0 both (the joint evaluation, the default), 1 expression, 2 gesture.  Definition:
 *   1  encoder_aud and encoder_exp run; no gesture-encoder launch is issued.  dsh_eval writes the expression columns [dim_pose, C) of eps
 *      exactly as the joint evaluation does and 0 to the gesture columns; dsh_sample returns the joint run's expression columns and
 *      exactly 0 in the gesture columns.
 *   2  encoder_aud and encoder_ges run, and the gesture encoder reads `expression` [B,T,expression_dim] (device fp32, standardised, the
 *      clean track) wherever the joint evaluation reads the expression encoder's x0 estimate, at every step; the expression encoder is
 *      not launched.  dsh_eval writes the gesture columns of eps and 0 to the expression columns; dsh_sample returns the sampled gesture
 *      columns and the given track, bit for bit, in the expression columns.  Given the joint evaluation's own estimate (dsh_debug_copy
 *      "expr_x0") the gesture columns are the joint evaluation's, bit for bit.
 * Tensors keep their full width [B,T,C] in every mode; the inactive columns of x, gt, mask and the noise are never read, and the result
 * never depends on what x held there.  Noise addressing (draw order, Philox counters, row keys, noise-stack offsets) and every decision
 * taken by token rows (sub-batch streams, kernel families, graph and timestep-cache range) stay those of the joint run of the same
 * (B, T); only the two-stream encoder pipeline is not entered: there is one chain.  dsh_eval_flops and the profiler count what was launched.
 * Lifetime: part of the condition.  Call it after dsh_set_condition / dsh_set_condition_ragged, which reset the modality to 0 — every call
 * sequence without it is unchanged.  `expression` is copied into context-owned memory in stream order (like the conditioning tensors)
 * and packed once per condition; with lengths set, frames beyond a clip's length are read as zero.  `expression` is ignored unless
 * modality is 2.
 * -1 before any state changes (the previous condition and modality stay usable) on an unknown value, on a single_transformer context
 * (modality != 0), before any dsh_set_condition, and on modality 2 with a null track.  dsh_sample returns -1 on same_overlap_noisy
 * with a partial modality (the saved noisy tails describe all channels); `trace` is allowed, inactive columns of its rows are unspecified. */
int dsh_set_modality(dsh_ctx* ctx, int32_t modality, const float* expression);
/* eps[B,T,C] = UniDiffuser(x[B,T,C], t[B]; sqrt_alphas = (c1[B], c2[B])).  t holds ORIGINAL-scale
 * timesteps (what _WrappedModel passes); c1/c2 are sqrt(1/abar_t), sqrt(1/abar_t - 1) per sample
 * (gaussian_diffusion.py:527-532).  All device pointers; asynchronous on the context stream. */
int dsh_eval(dsh_ctx* ctx, const float* x, const int64_t* t, const float* c1, const float* c2, float* eps);
/* GEMM + attention flops actually launched by the last dsh_eval (work skipped is not counted; a doubled CFG batch counts both halves). */
double dsh_eval_flops(const dsh_ctx* ctx);
/* Per-kernel-class HIP-event timing on the context stream (bench.py roofline leg).  enable=1 resets and
 * starts recording; dsh_profile_read synchronises and returns, per class, the summed milliseconds, launch
 * counts, algorithmic flops and algorithmic HBM bytes; every output array has 16 entries.
 * dsh_profile_class_info names class `cls`: the kernel as rocprofv3 prints it (empty string = unused class)
 * and its role in the denoiser (static strings). */
int dsh_profile_enable(dsh_ctx* ctx, int32_t enable);
int dsh_profile_read(dsh_ctx* ctx, double* ms16, int64_t* launches16, double* flops16, double* bytes16);
int dsh_profile_class_info(const dsh_ctx* ctx, int32_t cls, const char** kernel, const char** role);
/* debug taps after dsh_eval: "aud_feat" [B,T,audio_dim], "expr_x0" [B,T,expression_dim] (device out). */
int dsh_debug_copy(dsh_ctx* ctx, const char* what, float* out);

/* ---- boundary 2: full sampling loops ----------------------------------------------------------- */
/* One loop = one dsh_sampler_opts + one dsh_run_spec.  The spec carries everything a loop needs from its caller beside the options; the
 * context keeps NONE of it between calls (caches only: a caller that passes the same row keys again pays no second upload), so a call
 * depends on its arguments, the condition and the guidance scale alone, and a refused call leaves nothing behind.
 * Set struct_size = sizeof(dsh_run_spec) and zero the rest before filling in: fields are only ever appended, a library newer than the
 * caller reads the fields the caller does not know as 0 / NULL (their defaults), and a struct_size larger than the library knows is refused.
 * The fields are described at the compatibility entries below that used to carry them (dsh_sample and the dsh_sample_set_* setters). */
typedef struct dsh_run_spec {
    uint32_t struct_size;
    int32_t init;            /* 0 x_T is drawn, 1 x is given, 2 x holds x0 (dsh_sample: init_from_x)                           */
    int32_t masked;          /* the caller's `True in outpainting_mask`                                                         */
    int32_t start_level;     /* 0: the whole schedule; K: the DDIM loops start at spaced level K - 1 (dsh_sample_set_start_level) */
    int32_t invert_from;     /* the reverse loop (DDIM inversion, dsh_invert_from) over the levels invert_from .. invert_to - 1  */
    int32_t invert_to;       /* when invert_to > 0: no draws; init, masked, the noise fields, the solver and the row keys unread */
    float* x;                /* device [B,T,C], in/out                                                                          */
    const float* gt;         /* device [B,T,C] or NULL                                                                          */
    const uint8_t* mask;     /* device [B,T,C] or NULL                                                                          */
    const float* noise_stack;/* device [n_draws, B*T*C] for DSH_NOISE_STACK, else NULL                                          */
    int64_t n_draws;
    float* trace;            /* device [n_steps, B*T*C] or NULL                                                                 */
    const int32_t* timesteps;/* host: the free timestep subset (dsh_sample_set_timesteps); n_timesteps = 0: the 'ddimK' stride */
    int32_t n_timesteps;
    int32_t tail_blend;      /* dsh_sample_set_tail_blend                                                                       */
    const uint64_t* row_keys;  /* host, n_rows entries (dsh_sample_set_row_keys); n_rows = 0: one stream for the whole batch   */
    const uint64_t* row_seeds; /* host, n_rows entries or NULL (dsh_sample_set_row_seeds)                                      */
    int32_t n_rows;
    int32_t solver;          /* DSH_SOLVER_DDIM / DSH_SOLVER_DPM2M (dsh_sample_set_solver)                                      */
    /* Soft constraints while sampling (keyframe attraction, velocity / acceleration damping).  guidance = 0: none, the guide_* fields are
     * not read and every launch is what it is without them.  With L = the clip's length and z the guided signal of column c of clip b,
     *   log p = -1/2 sum_t W[b,t,c] (z[t] - Y[b,t,c])^2 - 1/2 vel[c] sum_{t=0..L-2} (z[t+1] - z[t])^2
     *           - 1/2 acc[c] sum_{t=1..L-2} (z[t+1] - 2 z[t] + z[t-1])^2,      g = guide_scale[level] * d log p / d z,
     * and every denoise step uses g where the reference uses cond_fn's value (condition_score in the DDIM loops, condition_mean in the
     * DDPM loop).  guide_space DSH_GUIDE_XT: z is the noisy sample, the reference's cond_fn(x, t) contract; DSH_GUIDE_X0: z is the step's
     * pred_xstart (after clip_denoised), the denoiser's Jacobian not applied.  Frames >= L have gradient 0.  No draw is added.
     * -1 before any state changes: with the reverse loop; on an unknown space; on n_guide_scale other than 0 or the run's level count
     * (respacing in the DDIM loops, diffusion_steps in the DDPM loop); on target / weight whose guide_batch / guide_frames /
     * guide_channels differ from the condition's [B, T, C], on vel / acc whose guide_channels differs from C. */
    int32_t guidance;
    int32_t guide_space;
    int32_t n_guide_scale;   /* 0: scale 1 at every level                                                                       */
    int32_t guide_batch, guide_frames, guide_channels;   /* the shape the caller built the guide tensors for                    */
    const float* guide_target; /* Y, device [B,T,C] or NULL (0)                                                                  */
    const float* guide_weight; /* W >= 0, device [B,T,C] or NULL (no attraction term)                                            */
    const float* guide_vel;    /* device [C] or NULL                                                                             */
    const float* guide_acc;    /* device [C] or NULL                                                                             */
    const float* guide_scale;  /* host, n_guide_scale entries, indexed by spaced level; a level with scale 0 runs unguided      */
    /* Synchronised window batches: every window of a long stream is one row of the batch, all rows run the plain DDIM loop together, and
     * behind every denoise step the L = sync_len frames row b shares with row sync_left[b] — the first L frames of b, the last L valid
     * frames of sync_left[b] — are reconciled in place by dsh_op_window_sync's arithmetic (one launch per step and chain, on the chain's own
     * columns; rows of `trace` are taken after it).  The caller supplies x_T (init = 1) with ONE noise value per stream frame, so both
     * copies of a shared frame stand at the same x_t at every level and the cross-fade of the updated values equals one step with the
     * cross-faded prediction.  n_sync = 0: off, no launch and no kernel argument is added anywhere.  The run is one chain (no sub-batch
     * streams); the two-encoder pipeline stays on.  -1 before any state changes: on n_sync other than the batch; on what
     * dsh_op_window_sync refuses, checked against the condition's lengths; with the DDPM loop, eta != 0, a mask, same_overlap_noisy,
     * tail_blend, a start level, the reverse loop, a noise stack (DSH_NOISE_STACK) and init != 1 — each would put per-window noise
     * into the shared frames. */
    const int32_t* sync_left;  /* host, n_sync entries: the row that holds this row's first sync_len frames as its tail; -1: none   */
    int32_t n_sync;            /* 0: off; else the batch                                                                         */
    int32_t sync_len;          /* the overlap L >= 1                                                                             */
} dsh_run_spec;
#define DSH_GUIDE_XT 0
#define DSH_GUIDE_X0 1
/* Runs the forward loops and the reverse loop.  Asynchronous on the context stream, except that new row keys / seeds are copied to the
 * device and waited for before the loop is queued (they are caller memory).  -1 before any state changes on everything dsh_sample and
 * dsh_invert_from refuse, with the same messages.  The sticky values of the dsh_sample_set_* setters are neither read nor changed. */
int dsh_sample_run(dsh_ctx* ctx, const dsh_sampler_opts* opts, const dsh_run_spec* spec);
/* Host only: the Gaussian tensors [B,T,C] the loop of (opts, spec) consumes, in the reference's draw order: x_T or the
 * q_sample noise first (unless init = 1), then per step; and its (denoise + undo) steps, i.e. the rows a trace needs.  Either output may
 * be NULL.  The pointers to device memory in spec are not read.  -1 on what dsh_sample_run would refuse without seeing a context. */
int dsh_sample_count(const dsh_sampler_opts* opts, const dsh_run_spec* spec, int64_t* n_draws, int64_t* n_steps);

/* ---- compatibility layer over dsh_sample_run: sticky setters, dsh_sample, dsh_invert, three generations of counting entries ----
 * Each setter stores its value in one spec-shaped record of the context; dsh_sample / dsh_invert_from complete that record with their
 * arguments and run it; the counting entries build a spec from theirs.  New code should fill a dsh_run_spec instead. */
/* Number of Gaussian tensors [B,T,C] the loop consumes, in the reference's draw order
 * (SURVEY §8a S7): x_T first (unless init_from_x), then per step.  Returns < 0 on error. */
/* (init_from_x here is a flag: any non-zero value counts as "x is given".  For init_from_x = 2 of dsh_sample - one draw more, the
 * q_sample noise - size the stack with dsh_sample_num_draws_from below.) */
int64_t dsh_sample_num_draws(const dsh_sampler_opts* opts, int32_t masked, int32_t init_from_x);
/* Number of (denoise + undo) steps, i.e. rows a trace buffer needs. */
int64_t dsh_sample_num_steps(const dsh_sampler_opts* opts, int32_t masked);
/* x[B,T,C] (device, in/out): start sample if init_from_x, final sample on return.
 * gt / mask (device, [B,T,C] fp32 / uint8) may be NULL; `masked` is the caller's
 * `True in outpainting_mask` (gaussian_diffusion.py:1126).  noise_stack: device fp32
 * [n_draws, B*T*C] for DSH_NOISE_STACK, else NULL.  trace (device, nullable): [n_steps, B*T*C],
 * receives the sample after every step.  Asynchronous on the context stream.  (Large batches are sampled as two or three
 * independent sub-batches, each running the whole loop on an internal stream forked from and joined to the context stream:
 * for the caller everything stays ordered on the context stream.  A clip's result does not depend on the sub-batch it was sampled
 * in as long as the sub-batch and the whole batch run the same kernels: bit-identical to one stream whenever both are on the same
 * side of the fused-FFN limit of 8192 token rows per launch (CFG-doubled rows included) - always with classifier-free guidance, where
 * a split batch (>= 12288 clip rows) and its halves are all above it.  Without doubling (guidance scale 1) a batch of 12288 .. 16383
 * rows is above the limit and its halves are below: the halves round the FFN hidden layer to bf16, the unsplit batch keeps it in
 * fp32, and the two agree to bf16 round-off only.  fp32 precision: always bit-identical.
 * Shapes: see dsh_set_condition - a shape it accepts is never refused here.) */
/* init_from_x = 2: x holds a clean motion x0.  Draw 0 - the draw x_T takes in a run from noise, with the same row keys, row seeds and
 * ragged lengths - is the q_sample noise: x <- sqrt(ac[k]) x0 + sqrt(1 - ac[k]) n at the first level k of the schedule (K-1 with a start
 * level), and the steps' draws follow from index 1 as in a run from noise.  DDIM loops only. */
int dsh_sample(dsh_ctx* ctx, const dsh_sampler_opts* opts, float* x, int32_t init_from_x, const float* gt,
               const uint8_t* mask, int32_t masked, const float* noise_stack, int64_t n_draws, float* trace);
/* DSH_NOISE_PHILOX only: give every batch row its own generator key (host array of n = B entries; n = 0 restores
 * the single whole-batch stream).  Row b then draws from key `seed` with the 128-bit Philox counter
 * (draw index and position inside the row, keys[b]): distinct (seed, key) pairs never share a stream, and the
 * counters depend only on the draw index and the position inside the row, so a chain identified by a global id
 * receives the same noise
 * whatever batch, stream split or rank it is sampled in (sharded test_arbitrary_len, ddpm_show_trainer.py:743-750:
 * the reference instead draws from each rank's global torch RNG).  Sticky until changed; frames*channels % 4 == 0. */
int dsh_sample_set_row_keys(dsh_ctx* ctx, const uint64_t* keys_host, int32_t n);
/* DSH_NOISE_PHILOX with row keys only: give every batch row its own Philox KEY as well (host array of n entries).  Row b then draws
 * from key seeds_host[b] wherever the loop uses opts->seed - x_T, every step's randn_like, the noise of the RePaint blend's gt, the undo
 * steps and the eta draws, on every stream the loop runs on - with the counter unchanged (draw index and position inside the row in
 * the low words, keys[b] in the high words; ragged rows advance by their own size as before).  A chain's window k is sampled with
 * the key hash(base seed, k), so rows standing at DIFFERENT windows of their chains (live sessions batched together) each draw exactly
 * what they draw alone in a call whose opts->seed is that hash.  Needs the row keys set, and n equal to their count: -1 before any state
 * changes otherwise.  Sticky like the keys; n = 0 clears it, and so does every dsh_sample_set_row_keys call (the seeds belong to the key
 * set they were given for: set the keys first, then the seeds).  Without row seeds every value is what it was, bit for bit. */
int dsh_sample_set_row_seeds(dsh_ctx* ctx, const uint64_t* seeds_host, int32_t n);
/* Windows pinned at BOTH ends (motion in-betweening, seam repair of multi-chain streams): the reference cross-fades generated motion
 * into the pinned frames on the first overlap_len frames only (addBlend, gaussian_diffusion.py:1051-1054).  on != 0 adds the mirror
 * image on the last overlap_len frames of every DDIM step the head fade runs in (add_blend set, noise weight < 0.2):
 *   g[t] = g[t] (1 - w'[j]) + s[t] w'[j],  j = t - (frames - L),  w'[j] = linspace(0, 1, L)[L - 1 - j]   (fp32, individually rounded)
 * before the mask select, so the last pinned frame is kept exactly (weight 0) and the fade grows towards the re-sampled middle.
 * on = 0 (the default) is the reference's loop, bit for bit.  Sticky until changed.  dsh_sample then returns -1 when
 * 2 * overlap_len > frames, and with same_overlap_noisy (the saved noisy tails describe a window chain). */
int dsh_sample_set_tail_blend(dsh_ctx* ctx, int32_t on);
/* ---- editing an existing motion: restart from a level, q_sample, DDIM inversion ----
 * Start level K of the DDIM loops, 1 <= K <= respacing (0, the default: the whole schedule, bit for bit).  The plain schedule becomes
 * the spaced levels K-1 .. 0; the mask-present (RePaint) schedule becomes the jump schedule walked from t_T = K in place of its
 * built-in 15 / 0.6 * respacing.  x enters at level K-1: given (init_from_x = 1), or built from a clean motion (init_from_x = 2, below).
 * Sticky like the tail blend.  dsh_sample then returns -1 on a DDPM loop, on K > respacing, with same_overlap_noisy and with the
 * tail blend. */
int dsh_sample_set_start_level(dsh_ctx* ctx, int32_t level);
/* dsh_sample_num_draws / _num_steps of a run with init mode `init` (0, 1 or 2) and start level `start_level`; the two entries above are
 * these with start_level = 0. */
int64_t dsh_sample_num_draws_from(const dsh_sampler_opts* opts, int32_t masked, int32_t init, int32_t start_level);
int64_t dsh_sample_num_steps_from(const dsh_sampler_opts* opts, int32_t masked, int32_t init, int32_t start_level);
/* DDIM inversion (ddim_reverse_sample, gaussian_diffusion.py:1068-1104): x [B,T,C] (device, in/out) is carried through the spaced levels
 * 0 .. to_level-1 of the reverse ODE in place, each step evaluating the model at level k and writing
 *   x <- sqrt(ac_next[k]) x0 + sqrt(1 - ac_next[k]) eps        (ac_next[k] = alphas_cumprod[k+1], 0 behind the last level)
 * with the DDIM step's kernel.  No draws; opts->kind must be DDIM and opts->eta 0; no mask; no start level, tail blend or
 * same_overlap_noisy (-1).  trace (device, nullable): [to_level, B*T*C].  The result stands at alphas_cumprod[to_level]; a decode
 * with start level K enters at alphas_cumprod[K-1] (the guided-diffusion pairing: not an exact inverse). */
int dsh_invert(dsh_ctx* ctx, const dsh_sampler_opts* opts, float* x, int32_t to_level, float* trace);
/* the same over the levels from_level .. to_level-1 (0 <= from_level < to_level; x enters at from_level): one reverse step is
 * (t, t+1).  trace: [to_level - from_level, B*T*C]. */
int dsh_invert_from(dsh_ctx* ctx, const dsh_sampler_opts* opts, float* x, int32_t from_level, int32_t to_level, float* trace);
/* ---- few-step sampling: free timestep subsets and the DPM-Solver++(2M) update ----
 * The DDIM loops and dsh_invert run on the original timesteps kept_host[0 .. n) instead of the 'ddimK' stride: strictly ascending,
 * >= 0 (-1 otherwise, and the previous list stays).  Tables: beta'_k = 1 - ac[kept_k] / ac[kept_{k-1}], timestep map = the list.
 * Sticky; n = 0 restores the stride.  With a list set, dsh_sample and dsh_invert return -1 before any state changes when
 * n != opts->respacing, when an entry is >= opts->diffusion_steps, and on a DDPM loop.  dsh_invert takes the list from the context; the
 * counting entries below take it as an argument.
 * Out-painting start: a list that is the 'ddimK' stride of its own length keeps the reference's rule t_T = 15 / int(0.6 K); any other
 * list starts a masked window at t_T = 1 + min{k : alphas_cumprod'[k] <= alphas_cumprod[14] of the ddim25 tables of the same
 * diffusion_steps} (dsh_masked_start_level), the noise level where the reference starts one.  dsh_sample_set_start_level overrides. */
int dsh_sample_set_timesteps(dsh_ctx* ctx, const int32_t* kept_host, int32_t n);
#define DSH_SOLVER_DDIM 0
#define DSH_SOLVER_DPM2M 1
/* Update rule of the DDIM loops.  DSH_SOLVER_DPM2M: a denoise step at level k is the second-order multistep update of
 * DPM-Solver++(2M) in the data-prediction form,
 *   x0 = c1 x - c2 eps (clamped when clip_denoised);  D = x0 + G (x0 - x0_prev);  x <- A x + Bc D;  then the RePaint branch,
 * if and only if the previous executed step of this run was the denoise step at level k + 1 and k != 0.  Every other step - the first of
 * a run (also one entered through a start level or init_from_x 1 / 2), the step after an undo step, the last step to alphas_cumprod_prev
 * = 1 - is the DDIM update bit for bit.  With respacing <= 2 the two solvers are the same loop.  Draws: those of the DDIM loop (same
 * count, indices and Philox offsets).  One extra [B,T,C] fp32 buffer in the context holds x0_prev.  Sticky; -1 on an unknown value.
 * dsh_sample then returns -1 before any state changes with eta != 0, with same_overlap_noisy and on a DDPM loop.  dsh_invert ignores the
 * solver: the reverse ODE stays the reference's first-order ddim_reverse_sample. */
int dsh_sample_set_solver(dsh_ctx* ctx, int32_t solver);
/* dsh_sample_num_draws_from / _num_steps_from for a run on the subset kept[0 .. n) (n = 0: the stride); -1 when n != opts->respacing.
 * The counts depend on n and, mask-present, on the start level above only. */
int64_t dsh_sample_num_draws_subset(const dsh_sampler_opts* opts, int32_t masked, int32_t init, int32_t start_level, const int32_t* kept, int32_t n);
int64_t dsh_sample_num_steps_subset(const dsh_sampler_opts* opts, int32_t masked, int32_t init, int32_t start_level, const int32_t* kept, int32_t n);
/* Classifier-free guidance scale of dsh_eval and dsh_sample (transformer.py:537, :586: eps = u + s_b (k - u) for clip b, in both motion
 * encoders; the expression x0 the gesture encoder reads is built from the mixed expression eps).  Host array of n entries: n = 0 restores
 * the config's cond_scale, n = 1 sets one value for the whole batch, n = B one value per clip (checked against the batch of
 * dsh_set_condition when dsh_eval / dsh_sample run: -1 on a mismatch).  Sticky until changed; copied in stream order into a device
 * buffer the context owns, which the kernels (and captured graphs) read when they run.  The null half is evaluated (the batch doubled)
 * only when the weights are classifier_free and some scale != 1; a clip at exactly 1 inside a doubled batch returns k itself.  Mixed
 * batches pay the full doubling.  -1 on a non-finite value, and on any value != 1 when the weights are not classifier_free. */
int dsh_set_guidance_scale(dsh_ctx* ctx, const float* scales_host, int32_t n);
/* Guidance schedule: the weight of the guidance per model timestep and per encoder, and the std rescale of the guided
 * prediction (Lin et al., "Common diffusion noise schedules and sample steps are flawed", guidance_rescale).  Host arrays of n_steps =
 * the model's diffusion_steps gains each (index = the ORIGINAL timestep, what dsh_eval takes as t), rescale factors phi in [0, 1].  Sticky
 * like the scale; n_steps = 0 clears it (the arrays are not read), and with no schedule set every evaluation issues the launches it
 * always did.  Per clip b and encoder m (expression / gesture) at the evaluation's timestep t_b, in fp32, every operation rounded to
 * nearest, no fma:
 *     s      = scale[b]                                   (dsh_set_guidance_scale)
 *     g      = gain_m[t_b]
 *     s_eff  = g == 1 ? s : 1 + g (s - 1)
 *     e      = s_eff == 1 ? k : u + s_eff (k - u)          (u / k: the unconditional / conditional prediction)
 * and, only where the batch is doubled, phi_m > 0 and s_eff != 1, over the clip's own valid elements (frames t < len_b, the encoder's w
 * columns; padded frames are never read), n = len_b w:
 *     f  = float(phi_m sigma_k / sigma_e + (1 - phi_m))    sigma: unbiased (n - 1) standard deviation, accumulated in fp64
 *          when n >= 2 and sigma_e is finite and > 0, else exactly 1
 *     e' = f e
 * The expression x0 the gesture encoder reads is c1 x - c2 e'.  The doubling rule of dsh_set_guidance_scale is unchanged: the null half is
 * evaluated if and only if the weights are classifier_free and some scale[b] != 1; in an undoubled batch the schedule is inert, and a gain
 * of 0 gives s_eff = 1 and takes k itself (the null half is still evaluated).  A modality run alone reads its own row.  The table is
 * copied in stream order into a device buffer the context owns at a fixed address, which the kernels (and captured graphs) read when
 * they run.  One launch per encoder and evaluation with phi_m = 0 (the launch count of the unscheduled mix), two with phi_m > 0.
 * -1 before any state changes on a non-finite gain, phi outside [0, 1], n_steps != diffusion_steps, a schedule other than all gains 1
 * with phi 0 on weights that are not classifier_free, and on a single_transformer context (one encoder) with two different rows or
 * two different phi. */
int dsh_set_guidance_schedule(dsh_ctx* ctx, const float* gain_expression, const float* gain_gesture, int32_t n_steps, float rescale_expression,
                              float rescale_gesture);

/* ---- schedule / table introspection (host; parity tests for S1-S3) ---------------------------- */
/* name in {betas, alphas_cumprod, alphas_cumprod_prev, sqrt_recip_alphas_cumprod,
 * sqrt_recipm1_alphas_cumprod, posterior_variance, posterior_log_variance_clipped,
 * posterior_mean_coef1, posterior_mean_coef2}; respacing 0 = full chain.  Returns entries written. */
int32_t dsh_diffusion_table(int32_t diffusion_steps, int32_t respacing, const char* name, double* out, int32_t cap);
/* the same tables for the subset kept[0 .. n) of original timesteps (strictly ascending, each in [0, diffusion_steps), n >= 1); the
 * 'ddimK' list gives dsh_diffusion_table(diffusion_steps, K, ...) bit for bit. */
int32_t dsh_diffusion_table_subset(int32_t diffusion_steps, const int32_t* kept, int32_t n, const char* name, double* out, int32_t cap);
/* out3 = {A, Bc, G} of dsh_sample_set_solver at spaced level k of that subset, fp64 (the loop casts them to fp32): with ab =
 * alphas_cumprod[k], abp = alphas_cumprod_prev[k], lambda(a) = log(a / (1 - a)) / 2 and h = lambda(abp) - lambda(ab),
 *   A = sqrt((1 - abp) / (1 - ab)),  Bc = -sqrt(abp) expm1(-h),  G = h / (2 (lambda(ab) - lambda(alphas_cumprod[k + 1]))).
 * G = 0 at k = 0 (h is infinite: A = 0, Bc = 1) and at k = n - 1: no second-order step exists there. */
int dsh_solver_coeffs(int32_t diffusion_steps, const int32_t* kept, int32_t n, int32_t k, double* out3);
/* t_T of a mask-present run on that subset (dsh_sample_set_timesteps); 0 = the reference's index rule (n = 0, or a 'ddimK' stride). */
int32_t dsh_masked_start_level(int32_t diffusion_steps, const int32_t* kept, int32_t n);
int32_t dsh_timestep_map(int32_t diffusion_steps, int32_t respacing, int32_t* out, int32_t cap);
int32_t dsh_jump_schedule(int32_t respacing, int32_t jump_length, int32_t jump_n_sample, int32_t* out, int32_t cap);

/* ---- rows either side of the path ---------------------------------------------------- */
/* y[B,frames_out,C] = F.interpolate(x^T, size=frames_out, mode='linear', align_corners=True)^T of x[B,frames_in,C]:
 * HuBERT hidden states resampled to the pose frame rate (datasets/show.py:98, ddpm_show_trainer.py:1082). */
int dsh_interp_time(void* hip_stream, const float* x, int32_t batch, int32_t frames_in, int32_t channels, float* y,
                    int32_t frames_out);
/* The same for a batch whose rows have frame counts of their own on both sides (DEVICE int32 [batch], clamped to frames_in / frames_out, the
 * padded sizes): row b is dsh_interp_time of its first lens_in[b] frames to lens_out[b] frames, bit for bit; y[b, t >= lens_out[b]] = 0.  No
 * frame >= lens_in[b] is read. */
int dsh_interp_time_ragged(void* hip_stream, const float* x, int32_t batch, int32_t frames_in, int32_t channels, float* y, int32_t frames_out,
                           const int32_t* lens_in_dev, const int32_t* lens_out_dev);
/* y = x * std[c] + mean[c] over n contiguous fp32 values with `channels` innermost (datasets/show.py:157-162). */
int dsh_inv_standardize(void* hip_stream, const float* x, int64_t n, int32_t channels, const float* mean, const float* stdv,
                        float* y);
/* BEAT results tail (trainers/ddpm_beat_trainer.py:1044-1060, :1318-1333, :811-817): the gesture channels of a sampled result are
 * standardised axis-angle vectors (--axis_angle); what the reference saves, scores and writes to BVH are standardised Euler 'XYZ' angles
 * in degrees.  Per row r < rows and joint j < joints, on the three values x[r * ld_x + 3 j ..]:
 *   v = x * std_aa + mean_aa -> quaternion -> rotation matrix -> Euler XYZ (datasets/rotation_converter.py:204-233, :251-280, :342-381)
 *   -> degrees -> y_deg[r * ld_deg + 3 j ..];  (deg - mean_e) / std_e -> y_std[r * ld_std + 3 j ..].
 * fp32, the reference's order of operations, accurate transcendentals.  One deviation: the asin argument is clamped to [-1, 1], so a joint
 * at gimbal lock gives +-90 degrees where the reference's fp32 run gives NaN when R02 rounds past 1.  Either output may be NULL (not
 * both).  Strides are in elements and >= 3 * joints: ld_x = 192, joints = 47 reads the gesture columns of a BEAT [B, T, 192] result in
 * place; columns behind 3 * joints are neither read nor written.  The four statistics are device fp32 [3 * joints].
 * lengths_dev (nullable, device int32 [rows / frames]; rows % frames == 0): row r belongs to clip r / frames at frame r % frames; rows at
 * frames >= lengths_dev[clip] are written as exact zeros in both outputs and never read (the ragged sampler's convention: padded frames
 * of a result are 0 - converting a zero pad would otherwise give -mean_e / std_e).  Asynchronous on hip_stream; a result does not depend
 * on the launch geometry.  -1: joints < 1, a stride below 3 * joints, a null input or statistics pointer, both outputs null, rows < 0,
 * lengths with frames < 1 or rows % frames != 0. */
int dsh_axis_angle_to_euler(void* hip_stream, const float* x, int64_t ld_x, int64_t rows, int32_t joints, const float* mean_aa,
                            const float* std_aa, const float* mean_e, const float* std_e, float* y_std, int64_t ld_std, float* y_deg,
                            int64_t ld_deg, const int32_t* lengths_dev, int32_t frames);
/* The inverse, the direction the dataset takes from BVH Euler data to its axis-angle targets (datasets/beat.py:376-401):
 *   deg = x * std_e + mean_e -> radians -> Rx Ry Rz (rotation_converter.py:147-173) -> quaternion (the candidate with the largest |q|
 *   component, 0.1 floor in the denominator, :44-103) -> axis-angle (:12-40; the angle may exceed pi, as in the reference)
 *   -> (aa - mean_aa) / std_aa -> y[r * ld_y + 3 j ..].
 * Strides, statistics, lengths_dev and refusals as above. */
int dsh_euler_to_axis_angle(void* hip_stream, const float* x, int64_t ld_x, int64_t rows, int32_t joints, const float* mean_e,
                            const float* std_e, const float* mean_aa, const float* std_aa, float* y, int64_t ld_y,
                            const int32_t* lengths_dev, int32_t frames);

/* Forward kinematics of a rotation-only skeleton: world-space joint positions of the gesture channels.  The skeleton is
 * the caller's, as DEVICE buffers whose contents this call does not validate: parents int32 [joints] (parents[0] = -1, parents[j] < j),
 * offsets fp32 [joints, 3] (a BVH's OFFSET lines, end sites included as joints), channel_joint int32 [channels] (channel triple i drives
 * joint channel_joint[i]; distinct), joint_channel int32 [joints] (the inverse map, -1 where no channel drives the joint), rest_rot fp32
 * [joints, 3, 3] row-major (the rotation of an undriven joint).  Per row r < rows, in fp32 without FMA contraction, every 3-term product
 * as (a0 b0 + a1 b1) + a2 b2:
 *   v_i = x[r * ld_x + 3 i ..] * stdv + mean              (kind 1, "euler": deg = x * stdv + mean -> radians -> Rx Ry Rz)
 *   R_j = exp([v_i]x) via the unit quaternion of dsh_axis_angle_to_euler (same small-angle series), j = channel_joint[i];
 *   R_j = rest_rot[j] otherwise
 *   W_0 = R_0,           p_0 = offsets[0]
 *   W_j = W_parent R_j,  p_j = p_parent + W_parent offsets[j]
 *   pos[r * ld_pos + 3 j ..] = p_j;  wrot[r * ld_wrot + 9 j ..] = W_j row-major (wrot may be NULL).
 * mean / stdv: device fp32 [3 * channels], the statistics of the input kind.  Strides in elements: ld_x >= 3 * channels (ld_x = 192,
 * channels = 47 reads a BEAT [B, T, 192] result in place), ld_pos >= 3 * joints, ld_wrot >= 9 * joints.  lengths_dev / frames exactly as
 * for dsh_axis_angle_to_euler: rows behind a clip's length are written as exact zeros and never read.  Asynchronous on hip_stream, no
 * atomics; a row's bits depend neither on the launch geometry nor on the rows around it.  -1 before any launch: joints outside
 * 1 .. DSH_FK_MAX_JOINTS, channels outside 1 .. joints, kind not 0 / 1, a null required pointer, a stride below its minimum, rows < 0,
 * lengths with frames < 1 or rows % frames != 0. */
#define DSH_FK_MAX_JOINTS 256
int dsh_fk_positions(void* hip_stream, const float* x, int64_t ld_x, int64_t rows, int32_t kind, const float* mean, const float* stdv,
                     int32_t joints, int32_t channels, const int32_t* parents, const float* offsets, const int32_t* channel_joint,
                     const float* rest_rot, const int32_t* joint_channel, float* pos, int64_t ld_pos, float* wrot, int64_t ld_wrot,
                     const int32_t* lengths_dev, int32_t frames);
/* The vector-Jacobian product of the positions above: given g = dL/dpos [rows, ld_g >= 3 * joints], dx[r * ld_dx + 3 i ..] = dL/dx
 * [rows, ld_dx >= 3 * channels].  kind must be 0 (axis-angle); kind 1 is refused.  The forward pass is recomputed per row; then F_j = g_j,
 * M_j = 0 and, for j = joints - 1 .. 1 with p = parents[j] (a fixed order: a joint's children are added in descending index order),
 *   M_p = M_p + (M_j + (p_j - p_p) x F_j),  F_p = F_p + F_j
 * so that M_j = sum over the strict descendants k of (p_k - p_j) x g_k.  Per driven joint, with u = W_j^T M_j and t = |v|:
 *   dL/dv = (u + a (v x u)) + b (v x (v x u)),  a = (1 - cos t) / t^2 evaluated as (sin(t/2) / (t/2))^2 / 2,  b = (t - sin t) / t^3;
 *   below t = 1e-3: a = 1/2 - t^2 / 24, b = 1/6 - t^2 / 120;     dL/dx = stdv * dL/dv
 * (the transposed right Jacobian of the exponential map).  Padded rows give exact zeros and neither x nor g is read there.  Other
 * arguments, guarantees and refusals as above. */
int dsh_fk_positions_vjp(void* hip_stream, const float* x, int64_t ld_x, int64_t rows, int32_t kind, const float* mean, const float* stdv,
                         int32_t joints, int32_t channels, const int32_t* parents, const float* offsets, const int32_t* channel_joint,
                         const float* rest_rot, const int32_t* joint_channel, const float* g, int64_t ld_g, float* dx, int64_t ld_dx,
                         const int32_t* lengths_dev, int32_t frames);

/* ---- unit kernels (device pointers; used by the kernel-level parity tests) -------------------- */
/* C[M,N] = act(A[M,K] W[N,K]^T + bias) (+ R); dtype 0: fp32 operands, 1: bf16 operands (uint16 bits).
 * K must be a multiple of 32 (fp32) / 64 (bf16).  Cf: fp32 out (nullable); Ct: operand-typed out (nullable). */
int dsh_op_gemm(void* hip_stream, int32_t dtype, const void* A, const void* W, const float* bias, const float* R,
                float* Cf, void* Ct, int32_t M, int32_t N, int32_t K, int32_t act);
/* The same launch with every field of its argument block given by the caller, as the denoiser fills it: leading dimensions (elements) of
 * A, W, R, Cf and Ct; res_mod > 0 takes the residual from row m % res_mod (0: row m); act_after_res != 0 applies the activation behind
 * the residual, act(A W^T + bias + R).  Cf and Ct may both be given (Ct = the rounded Cf) and R may alias Cf.  Refused: no output, a
 * leading dimension below K (A, W) or N (R, Cf, Ct), a negative res_mod, an unknown act, A or W not 16-byte aligned. */
int dsh_op_gemm_ex(void* hip_stream, int32_t dtype, const void* A, const void* W, const float* bias, const float* R, float* Cf, void* Ct,
                   int32_t M, int32_t N, int32_t K, int32_t act, int32_t lda, int32_t ldw, int32_t ldr, int32_t res_mod, int32_t ldcf,
                   int32_t ldct, int32_t act_after_res);
/* fp32 parity path: a Linear with what the reference computes in front of it, in ONE launch (gemm_f32_pro.hip).
 *   pro 1: C = act(LayerNorm(concat(x0 .. x3)) W^T + b) with the LayerNorm affine FOLDED by the caller: W = gamma (.) W_ref, bias = b + W_ref beta,
 *          fc[n] = sum_k W[n][k]  (models/transformer.py:106-108,119-125 q|k|v; :284-289,304-312 feat_proj.0/.1).  Segment j is fp32 [M, ld_j], w_j
 *          columns wide (multiples of 32; zero padded where the real width is smaller); sum w_j = K; LayerNorm over the first k_real columns.
 *   pro 2: C = Linear(SiLU(LN(x0) scale' + shift')) + R, the StylizationBlock (models/transformer.py:86-97), film [nb, >= film_off + 2K] holding
 *          (scale' | shift') = (gamma (1 + scale) | beta (1 + scale) + shift) per sample, sample = (row / frames) % nb; K = ld-free width of x0.
 *   pro 0: C = act(x0 W^T + b) (+ R): the same software-pipelined main loop without a front.
 * Row moments travel between launches instead of being recomputed: stats_out (nullable, N % 64 == 0, N <= 512) receives [M][N / 32] pairs
 * (mean_g, sum (c - mean_g)^2) over groups of 32 output columns; stats (pro 2, nullable) takes such pairs for the INPUT rows, stat_groups groups
 * of K / stat_groups columns each, combined in a fixed order — the launch then makes no pass over its rows for the LayerNorm.
 * All pointers device fp32; W [N, K] row-major; R nullable [M, N]; C [M, N]. */
int dsh_op_gemm_f32_pro(void* hip_stream, int32_t pro, const float* x0, int32_t ld0, int32_t w0, const float* x1, int32_t ld1, int32_t w1,
                        const float* x2, int32_t ld2, int32_t w2, const float* x3, int32_t ld3, int32_t w3, int32_t k_real, const float* W,
                        const float* bias, const float* fc, const float* film, int32_t film_ld, int32_t film_off, int32_t frames, int32_t nb,
                        const float* R, float* C, int32_t M, int32_t N, int32_t act, const float* stats, int32_t stat_groups, float* stats_out);
/* The same launch with the main loop chosen: mma 0 = dsh_op_gemm_f32_pro (exact-fp32 MFMA), bit for bit; mma 1 = the split-bf16 loop of
 * DSH_PRECISION_BF16X3 (gemm_f32_split.hip): W (fp32, as above) is packed into hi / lo bf16 pieces in per-call scratch, the rows are split in the
 * launch's staging registers; pro 1 subtracts the mean of the row's first 32 columns before the split.  mma 1 + 16 t forces the split loop's
 * tile (t = 1: 64 x 64, t = 2: 128 x 128; the bits do not depend on it).  The split loop does not carry the row-moment side channel: stats and
 * stats_out must be null with mma 1.  + 64 (measurements): W is the packed operand already, as dsh_op_split_pack_weight left it - the call is
 * then the launch alone, without scratch and without a synchronisation, which is how the model issues it. */
/* The split loop's one weight packer: W fp32 [N, K] row-major (K a multiple of 32) -> out, N x K 32-bit words (16-byte aligned): per K tile of
 * 32 columns the 32 hi pieces, then the 32 lo pieces, hi = RNE_bf16(w), lo = RNE_bf16(w - hi).  Enqueued on the stream. */
int dsh_op_split_pack_weight(void* hip_stream, const float* W, int32_t N, int32_t K, void* out);
int dsh_op_gemm_f32_pro_ex(void* hip_stream, int32_t pro, const float* x0, int32_t ld0, int32_t w0, const float* x1, int32_t ld1, int32_t w1,
                           const float* x2, int32_t ld2, int32_t w2, const float* x3, int32_t ld3, int32_t w3, int32_t k_real, const float* W,
                           const float* bias, const float* fc, const float* film, int32_t film_ld, int32_t film_off, int32_t frames, int32_t nb,
                           const float* R, float* C, int32_t M, int32_t N, int32_t act, const float* stats, int32_t stat_groups, float* stats_out,
                           int32_t mma);
/* Token-per-lane fused Linear (bf16, K = 512 or 1024): out = act(prologue(X) W^T + bias) (+ R).  X bf16 [M,K]
 * with M padded to a multiple of 128 rows, W bf16 [N,K] in natural k order (permuted internally into a scratch
 * copy), pro 0 plain / 1 LayerNorm / 2 LayerNorm+FiLM+SiLU with film [nb, 2K] = (scale | shift) per sample,
 * sample = (row / frames) % nb; pro 3 (K = 1024): X is the row-major concat row [h 512 | audio_proj 256 | hubert 128 | expr 128]
 * of feat_proj.0 (transformer.py:304-312), LayerNorm over its first `frames` (= real width, 896 .. 1024) columns, gamma / beta
 * [1024] zero beyond them. */
/* Test helper: which kernel family the LAST token-per-lane Linear launch of this process selected — 0 = tl2 round-2 loop, 1 = tl2 rolling
 * loop, 2 = tl2 rolling loop on hi / lo residual planes, 10 = tl_linear (first generation), 11 = tl_small (window chain); -1 before any
 * launch.  Values 3, 4 and 5 are retired (kernel forms that were removed) and never returned.  Lets the bit-identity tests assert that
 * the kernel they mean to check is the one that ran. */
int32_t dsh_debug_last_tl_variant(void);
/* Test helper: launches issued by this process since the last reset, per kernel family (host-side counters: no kernel and no launch
 * argument knows about them).  Copies min(cap, n) entries into out (nullable), zeroes all of them afterwards when reset != 0, returns n.
 * Fixed indices (new ones are appended):
 *    0 tl_linear (first generation)        1 tl2 round-2 loop                    2 tl2 rolling loop
 *    3 tl2 rolling loop on hi / lo planes  4 retired, always 0                   5 tl_small (window chain)
 *    6 fused FFN launch (tl3_ffn / tl2_ffn)            7 retired, always 0
 *    8 bf16 layers: MFMA tiled attention               9 bf16 layers: row-major attention fallback (windows of more than 96 frames)
 *   10 fp32 few-row (K-split) GEMM        11 fp32 tiled GEMM                    12 gemm_f32_pro (exact-fp32 main loop only)
 *  and four VALUES rather than counts: 13 sub-batch streams of the last dsh_eval, 14 sub-batch streams of the last dsh_sample,
 *   15 whether the last dsh_sample replayed captured graphs, 16 whether it ran the two-encoder pipeline;
 *  two more counts: 17 weight-streaming GEMV (at most 16 rows, fp32 and bf16), 18 bf16 tiled GEMM;
 *  and one more value: 19 tile shape of the last tiled GEMM launch (0 128 x 128, 1 128 x 64, 2 64 x 64, 3 64 x 32, 4 the unswizzled
 *   128 x 128 form of DSH_GEMM_VARIANT=0);
 *  and two more counts: 20 gemm_f32_pro split-bf16 launches (DSH_PRECISION_BF16X3, dsh_op_gemm_f32_pro_ex with mma 1), both tile shapes;
 *   21 those of them that took the 128 x 128 instantiation. */
#define DSH_LAUNCH_COUNT_ENTRIES 22
int32_t dsh_debug_launch_counts(int64_t* out, int32_t cap, int32_t reset);
/* Test helper: the regime a sampling loop would take, from plain values — no context, no GPU call, no environment read.  dsh_sample_run
 * decides through the same function (csrc/loop_regime.h), once per run, from the facts it gathers itself.  Both structs start with
 * struct_size like dsh_run_spec: fields are only ever appended, unknown ones read as 0, a larger struct than the library knows is refused.
 *   facts   kind 0 DDIM (the reverse loop included) / 1 DDPM; batch, frames, channels; gesture_cols (-1: a single transformer); modality;
 *           evals / distinct_levels of the schedule (DDIM); trace, same_overlap_noisy, sync (synchronised windows), profiling as 0 / 1;
 *           cur_split = sub-batch streams the context is conditioned on before the loop; the switches as their readers see them:
 *           no_graph (DSH_NO_GRAPH present), level_cache, level_prefetch, pipe, graph_rows, and DSH_PIPE_ROWS twice — as the context
 *           read it when it was created and as the process latched it for the sampler
 *   regime  unsplit (the batch is conditioned as one batch), chains (1, or n sub-batch streams), forked_evals (one chain whose evaluations
 *           fork over the sub-batch streams), graph, cache (0 none, 1 inline, 2 side-stream prefetch, 3 inline per sub-batch stream),
 *           inline_ok (a failed prefetch falls back to the inline cache), pipe (the two encoders on two streams) */
typedef struct dsh_loop_facts {
    uint32_t struct_size;
    int32_t kind, batch, frames, channels, gesture_cols, modality;
    int32_t evals, distinct_levels;
    int32_t trace, same_overlap_noisy, sync, profiling;
    int32_t cur_split;
    int32_t no_graph, level_cache, level_prefetch, pipe;
    uint64_t graph_rows, pipe_rows_context, pipe_rows_sampler;
} dsh_loop_facts;
typedef struct dsh_loop_regime {
    uint32_t struct_size;
    int32_t unsplit, chains, forked_evals, graph, cache, inline_ok, pipe;
} dsh_loop_regime;
int dsh_debug_loop_regime(const dsh_loop_facts* facts, dsh_loop_regime* regime);
int dsh_op_tl_linear(void* hip_stream, int32_t pro, const void* X, const void* W, const float* bias, const float* R,
                     float* Cf, void* Ct, int32_t M, int32_t N, int32_t act, const float* gamma, const float* beta,
                     const float* film, int32_t frames, int32_t nb, int32_t K);
/* FFN branch of a decoder layer in one launch (bf16 path, latent 512 / ff 1024; models/transformer.py:169-181, :86-97):
 *   Cf = Hres + Linear3(SiLU(LN(y2; gamma, beta) * (1 + scale) + shift)) (+ row_const on rows < n_const_rows),
 *   y2 = GELU(X W1^T + b1) W2^T + b2;  Ct = bf16(Cf).  X bf16 [M,512], Hres / Cf fp32 [M,512], W1 [1024,512], W2 [512,1024],
 * W3 [512,512] bf16 row-major (natural order), film [nb, 1024] = (scale | shift) per sample, sample = (row / frames) % nb. */
int dsh_op_tl2_ffn(void* hip_stream, const void* X, const float* Hres, const void* W1, const float* b1, const void* W2, const float* b2,
                   const void* W3, const float* b3, const float* gamma, const float* beta, const float* film, int32_t frames, int32_t nb,
                   const float* row_const, int32_t n_const_rows, float* Cf, void* Ct, int32_t M);
/* Fused front of the bf16 path, one kernel each (test helpers like the two above: row-major device operands in natural order, packed with
 * the library's own packers in per-call scratch, nothing cached).
 * encoder_aud behind its attention (models/transformer.py:730-739): h = X2 + Ls1(SiLU(LN(Y; g1, be1) (1 + scale1) + shift1)),
 *   y2 = GELU(bf16(h) w1^T + b1) w2^T + b2, out = h + Ls2(SiLU(LN(y2; g2, be2) (1 + scale2) + shift2)); out_f fp32 [Mc,128], out_b = bf16(out)
 *   with leading dimension ld_b.  Y bf16 [Mc,128], X2 fp32 [Mc,128]; ws1 / ws2 [128,128], w1 [1024,128], w2 [128,1024] and their biases fp32
 *   (torch layouts); film [nb, 512] = (scale1 | shift1 | scale2 | shift2) of embedding row (row / frames) % nb. */
int dsh_op_tl_aud_tail(void* hip_stream, const void* Y, const float* X2, const float* ws1, const float* bs1, const float* w1, const float* b1,
                       const float* w2, const float* b2, const float* ws2, const float* bs2, const float* g1, const float* be1, const float* g2,
                       const float* be2, const float* film, int32_t frames, int32_t nb, int32_t Mc, float* out_f, void* out_b, int32_t ld_b);
/* audio_proj of one or two motion encoders: out_e = bf16(X W[e]^T + bias[e]); X bf16 [Mc,256], W fp32 [n_enc,256,256], bias fp32 [n_enc,256],
 * out0 / out1 bf16 row-major [Mc,256] (out1 null for n_enc == 1). */
int dsh_op_tl_aproj(void* hip_stream, const void* X, const float* W, const float* bias, int32_t n_enc, void* out0, void* out1, int32_t Mc);
/* Layer-0 seed: h = bf16(x[:, c0 : c0 + w]) bf16(Wj)^T + bias + pe[row % frames], as hi + lo planes read back in fp32.  x fp32 [Mc, ldx],
 * Wj fp32 [512, w] (w in 97 .. 112 or 129 .. 144), pe fp32 [frames, 512].  cnull == null: h_out [round_up(Mc, 32), 512], rows [0, Mc) = h.
 * cnull [512]: h_out [row1 + round_up(Mc, 32), 512], rows [0, Mc) = h + cnull (CFG-null half), rows [row1, row1 + Mc) = h; row1 a
 * multiple of 32, >= Mc.  Rows no kernel block covers come back as 0; the padding rows of a covered block are unspecified. */
int dsh_op_tl_joint(void* hip_stream, const float* x, int32_t ldx, int32_t c0, int32_t w, const float* Wj, const float* bias, const float* pe,
                    int32_t frames, const float* cnull, int32_t Mc, int32_t row1, float* h_out);
/* LinearTemporalCrossAttention (models/transformer.py:133-166; the `transformer_decoder` layer's ca_block): device fp32
 * weights under the module's own parameter names.  y = x + proj_out(softmax_ch(Wq LN(x)) (softmax_N(Wk tn(xf))^T Wv tn(xf)), emb),
 * x [B,T,D], xf [B,N,L], emb [B,E] (the raw embedding: proj_out.emb_layers applies SiLU first), y [B,T,D]. */
typedef struct dsh_cross_attn_weights {
    const float *norm_g, *norm_b;             /* norm            [D]      */
    const float *text_norm_g, *text_norm_b;   /* text_norm       [L]      */
    const float *wq, *bq;                     /* query           [D,D],[D] */
    const float *wk, *bk;                     /* key             [D,L],[D] */
    const float *wv, *bv;                     /* value           [D,L],[D] */
    const float *sty_norm_g, *sty_norm_b;     /* proj_out.norm   [D]      */
    const float *sty_emb_w, *sty_emb_b;       /* proj_out.emb_layers.1 [2D,E],[2D] */
    const float *sty_out_w, *sty_out_b;       /* proj_out.out_layers.2 [D,D],[D]   */
} dsh_cross_attn_weights;
int dsh_op_cross_attention(void* hip_stream, const dsh_cross_attn_weights* w, const float* x, const float* xf, const float* emb,
                           int32_t B, int32_t T, int32_t N, int32_t D, int32_t L, int32_t E, int32_t num_head, float* y);
/* y[nb,T,D] = linear attention core on qkv[nb,T,3D] (fp32), head_dim in {16,64}. */
int dsh_op_linear_attention(void* hip_stream, const float* qkv, int32_t nb, int32_t frames, int32_t D, int32_t head_dim,
                            float* y);
/* same on bf16 storage (uint16 bits in/out); head_dim 64 and frames <= 96 take the MFMA kernel. */
int dsh_op_linear_attention_bf16(void* hip_stream, const void* qkv, int32_t nb, int32_t frames, int32_t D, int32_t head_dim,
                                 void* y);
/* The same cores on a ragged batch: clip b has lens_dev[b % n_lens] valid frames (device int32; nb = n_lens, or 2 * n_lens for a
 * CFG-doubled batch whose halves share the lengths); frames beyond them enter neither the K softmax nor k^T v, every query row is still
 * answered.  lens_dev = NULL: the plain launch.  dtype 0 fp32 / 1 bf16 (uint16 bits).  variant 0: the kernel the denoiser's dispatch
 * selects for the shape (bf16, head_dim 64, <= 96 frames: the tiled MFMA kernel through scratch conversions); 1: bf16 on the row-major
 * kernels; 2: fp32 with the StylizationBlock front in the launch (D = 512, head_dim 64, <= 64 frames): y = SiLU(LN(attention) scale' +
 * shift') with film [n_lens, 2D] = (scale' | shift') per clip (LayerNorm affine folded in by the caller). */
int dsh_op_linear_attention_ragged(void* hip_stream, int32_t dtype, int32_t variant, const void* qkv, int32_t nb, int32_t frames, int32_t D,
                                   int32_t head_dim, void* y, const int32_t* lens_dev, int32_t n_lens, const float* film);
/* The tiled bf16 MFMA kernel alone (D % 64 == 0, 64-channel heads, <= 96 frames) through the same scratch conversions, with its two
 * launch arguments that no other entry reaches: the batch is laid out as n_half clips, a block-aligned gap, then the other nb - n_half
 * (the CFG halves of the denoiser), and rev = 1 walks the clips in descending order (the result is the same, bit for bit).  With
 * lens_dev: n_half = n_lens and nb = n_lens or 2 * n_lens. */
int dsh_op_linear_attention_tiled(void* hip_stream, const void* qkv, int32_t nb, int32_t n_half, int32_t frames, int32_t D, void* y,
                                  const int32_t* lens_dev, int32_t n_lens, int32_t rev);
/* out = LayerNorm(x[M,D]) * gamma + beta */
int dsh_op_layernorm(void* hip_stream, const float* x, int32_t M, int32_t D, const float* gamma, const float* beta,
                     float* out);
/* one launch of the sampler's fused DDIM step (eta = 0) on caller-supplied device buffers [B, frames, channels]: x in/out, eps the
 * model output; mask (bytes, null = no RePaint blend) with gt and noise2 (the N(0,1) of the noised gt); blend / tail_blend as
 * dsh_sampler_opts.add_blend (at a faded step) / dsh_sample_set_tail_blend; [c_lo, c_hi) restricts the update to a channel
 * range (0, 0 = all).  Asynchronous on hip_stream. */
int dsh_op_ddim_step(void* hip_stream, float* x, const float* eps, const float* gt, const uint8_t* mask, const float* noise2,
                     int32_t B, int32_t frames, int32_t channels, float c1, float c2, float sqrt_ab_prev, float sqrt_1m_ab_prev,
                     int32_t overlap_len, int32_t blend, int32_t tail_blend, int32_t clip, int32_t c_lo, int32_t c_hi);
/* standard normals from the on-device Philox generator */
int dsh_op_philox_randn(void* hip_stream, float* out, int64_t n, uint64_t seed, uint64_t offset);
/* q_sample (gaussian_diffusion.py:434-462): out[b] = a[b] x0[b] + s[b] n[b] over [B, frames, channels] (device fp32; out may be x0), every
 * product and the sum rounded on their own.  a_dev / s_dev: device arrays [B], one coefficient pair per row.  n = noise (device), or, when
 * noise is NULL, drawn inside the same pass: row_keys_host NULL = the values dsh_op_philox_randn(seed, offset) writes; else those of
 * dsh_op_philox_randn_rows (row_seeds_dev: _seeded; row_lens_host + draw: _ragged) for the same arguments.  Columns outside
 * [c_lo, c_hi) are not written (c_hi <= c_lo: all are); columns >= fixed_from are copied from x0 (-1: none; the reference's fix_head_var,
 * 24 / 90 for its two datasets); with row_lens_host, frames >= row_lens_host[b] of row b are written as 0. */
int dsh_op_q_sample(void* hip_stream, float* out, const float* x0, const float* noise, const float* a_dev, const float* s_dev, int32_t B,
                    int32_t frames, int32_t channels, int32_t c_lo, int32_t c_hi, int32_t fixed_from, uint64_t seed, uint64_t offset,
                    const uint64_t* row_keys_host, const uint64_t* row_seeds_dev, const int32_t* row_lens_host, uint64_t draw);
/* keep mask of an edit: keep [B, T, C] (device uint8) = 0 where frame t lies in one of row b's nf half-open frame ranges
 * frames[b, j] = (lo, hi) or column c in one of the nc column ranges cols[j] = (lo, hi), 1 elsewhere; one launch.  Both range lists are
 * given as a host copy (validated: 0 <= lo <= hi <= T / C, -1 otherwise) and a device copy (read by the kernel, which skips a range outside
 * those bounds all the same). */
int dsh_op_region_mask(void* hip_stream, const int32_t* frames_host, const int32_t* frames_dev, int32_t nf, const int32_t* cols_host,
                       const int32_t* cols_dev, int32_t nc, int32_t B, int32_t T, int32_t C, uint8_t* keep);
/* the per-row streams dsh_sample draws from after dsh_sample_set_row_keys: out[rows, n_row] (device), row b = key `seed`,
 * counter (offset + position inside the row, row_keys_host[b]); n_row % 4 == 0.  Synchronises the stream. */
int dsh_op_philox_randn_rows(void* hip_stream, float* out, int32_t rows, int64_t n_row, uint64_t seed, uint64_t offset,
                             const uint64_t* row_keys_host);

/* ---- one entry per small kernel of the sampler and around the denoiser (test helpers) --------------------------------------------
 * Device pointers in natural row-major order unless a name ends in _host; tiled results are read back through the library's own
 * untile launches into row-major buffers; nothing is cached.  Asynchronous on hip_stream unless stated.  -1 on a refused argument. */
/* dsh_op_philox_randn_rows with the ragged form the sampling loop uses: row_lens_host (nullable, [rows]) and channels > 0 make row b
 * advance by row_lens_host[b] * channels / 4 counters per draw (counter = draw * that + quad inside the row; `offset` is then unused).
 * Refuses a length whose row_lens * channels exceeds n_row.  Synchronises the stream. */
int dsh_op_philox_randn_rows_ragged(void* hip_stream, float* out, int32_t rows, int64_t n_row, uint64_t seed, uint64_t offset,
                                    const uint64_t* row_keys_host, const int32_t* row_lens_host, uint64_t draw, int32_t channels);
/* dsh_op_philox_randn_rows with the per-row Philox keys of dsh_sample_set_row_seeds: row_seeds_dev (DEVICE array [rows], nullable) gives
 * row b the key row_seeds_dev[b] in place of `seed`; NULL is dsh_op_philox_randn_rows itself.  Synchronises the stream. */
int dsh_op_philox_randn_rows_seeded(void* hip_stream, float* out, int32_t rows, int64_t n_row, uint64_t seed, uint64_t offset,
                                    const uint64_t* row_keys_host, const uint64_t* row_seeds_dev);
/* ... and its ragged sibling: dsh_op_philox_randn_rows_ragged with row_seeds_dev (DEVICE array [rows], nullable). */
int dsh_op_philox_randn_rows_ragged_seeded(void* hip_stream, float* out, int32_t rows, int64_t n_row, uint64_t seed, uint64_t offset,
                                           const uint64_t* row_keys_host, const int32_t* row_lens_host, uint64_t draw, int32_t channels,
                                           const uint64_t* row_seeds_dev);
/* Window hand-off of live chains on a device-resident slot table tails [S, L, C] (fp32, standardised motion: slot s holds the last
 * L = overlap_len frames of the window its chain sampled last).  Row r of a window batch belongs to slot slot_idx[r]; the index list is
 * given twice, as the host copy the call validates and the device copy the kernel reads (the kernel skips a row whose device index is
 * outside the table).  One launch each, plain loads and stores, any C, any T > L >= 1, asynchronous on hip_stream; R = 0 launches nothing.
 * -1 before any launch on L < 1, L >= T, a slot index outside [0, S) and - where slots are written - a slot named twice.
 * dsh_op_chain_handoff builds the reference's inpaint dictionary of a chained window (ddpm_show_trainer.py:889-893):
 *   gt [R, T, C]: gt[r, :L] = tails[slot_idx[r]], other frames 0;  mask [R, T, C] uint8: 1 on the first L frames, 0 elsewhere. */
int dsh_op_chain_handoff(void* hip_stream, const float* tails, int32_t S, const int32_t* slot_idx_host, const int32_t* slot_idx_dev,
                         int32_t R, int32_t T, int32_t L, int32_t C, float* gt, uint8_t* mask);
/* tails[slot_idx[r]] = x[r, n_r - L : n_r] for x [R, T, C], n_r = lens[r] (host and device copy, both or neither; L <= n_r <= T) or T. */
int dsh_op_chain_save_tail(void* hip_stream, const float* x, const int32_t* lens_host, const int32_t* lens_dev, const int32_t* slot_idx_host,
                           const int32_t* slot_idx_dev, int32_t R, int32_t T, int32_t L, int32_t C, float* tails, int32_t S);
/* Synchronised window batches (dsh_run_spec.sync_left): x [B, frames, channels] in place.  For every row b with p = left[b] >= 0, every
 * j < L and every column c of [c_lo, c_hi) ((0, 0): all; columns outside keep their bits), with n_p = lens[p] (or frames without lengths):
 *   a = x[p, n_p - L + j, c], r = x[b, j, c], w = linspace(0, 1, L)[j] (fp32, torch.linspace's values):
 *   x[p, n_p - L + j, c] = x[b, j, c] = a * (1 - w) + r * w          (every product and sum rounded on its own)
 * One launch, plain loads and stores, no atomics, asynchronous on hip_stream.  left and lens are given twice, as the host copies the call
 * validates and the device copies the kernel reads (the kernel skips a row whose device index or length is out of range).
 * -1 before any launch on: L < 1; left[b] outside -1 .. B - 1; left[b] = b; a row named as left neighbour twice; a row
 * that shares frames with a length below L or above frames; a row that shares frames at both ends with a length below 2 L; a column
 * range outside [0, channels]. */
int dsh_op_window_sync(void* hip_stream, float* x, int32_t B, int32_t frames, int32_t channels, const int32_t* left_host,
                       const int32_t* left_dev, const int32_t* lens_host, const int32_t* lens_dev, int32_t L, int32_t c_lo, int32_t c_hi);
/* dsh_op_ddim_step with every field of the step: x0_out (nullable) receives pred_xstart; coef_eps multiplies the re-derived eps and
 * sigma * noise1 is added when noise1 != NULL (the eta branch; eta = 0: coef_eps = sqrt_1m_ab_prev, noise1 = NULL); tail_in / tail_out
 * [B, overlap_len, channels] (nullable) are the saved noisy tail of --same_overlap_noisy.  Refusals of dsh_op_ddim_step, and tail_in
 * without a mask. */
int dsh_op_ddim_step_full(void* hip_stream, float* x, const float* eps, float* x0_out, const float* gt, const uint8_t* mask, const float* noise2,
                          const float* noise1, const float* tail_in, float* tail_out, int32_t B, int32_t frames, int32_t channels, float c1,
                          float c2, float sqrt_ab_prev, float sqrt_1m_ab_prev, float coef_eps, float sigma, int32_t overlap_len, int32_t blend,
                          int32_t tail_blend, int32_t clip, int32_t c_lo, int32_t c_hi);
/* One step of the DPM2M solver (dsh_sample_set_solver) on x [B, frames, channels] in place.  second_order != 0: the update above with
 * A, Bc, G (dsh_solver_coeffs, cast to fp32); x0_prev [B, frames, channels] holds the previous step's x0 and receives this step's in the
 * same pass.  second_order = 0: dsh_op_ddim_step_full at eta = 0 with x0_out = x0_prev (A, Bc, G unused).  mask / gt / noise2, blend,
 * tail_blend, clip and the channel range [c_lo, c_hi) as in dsh_op_ddim_step; columns outside the range are not touched in x or x0_prev. */
int dsh_op_dpm2m_step(void* hip_stream, float* x, const float* eps, float* x0_prev, const float* gt, const uint8_t* mask, const float* noise2,
                      int32_t B, int32_t frames, int32_t channels, float c1, float c2, float sqrt_ab_prev, float sqrt_1m_ab_prev, float A, float Bc,
                      float G, int32_t second_order, int32_t overlap_len, int32_t blend, int32_t tail_blend, int32_t clip, int32_t c_lo, int32_t c_hi);
/* x0 = c1 x - c2 eps (clamped when clip); x <- coef1 x0 + coef2 x + sigma noise on n values; [c_lo, c_hi) of `channels` restricts the
 * update (c_hi <= c_lo: all); x0_out nullable. */
int dsh_op_ddpm_step(void* hip_stream, float* x, const float* eps, const float* noise, float* x0_out, int64_t n, float c1, float c2, float coef1,
                     float coef2, float sigma, int32_t clip, int32_t channels, int32_t c_lo, int32_t c_hi);
/* The guidance terms of one launch (dsh_run_spec's guide_* fields, for one step): all device pointers but lens_host; any of target,
 * weight, vel, acc may be NULL (weight NULL: no attraction term; target NULL: 0).  lens_dev / lens_host [B]: per-clip frame counts in
 * 1 .. frames, both or neither. */
typedef struct dsh_guide {
    const float* target; const float* weight; const float* vel; const float* acc;
    const int32_t* lens_dev; const int32_t* lens_host;
    float scale;
    int32_t space;           /* DSH_GUIDE_XT / DSH_GUIDE_X0 (read by the two step entries) */
} dsh_guide;
/* g [B, frames, channels] = scale * d log p / d z for z [B, frames, channels] (the formula at dsh_run_spec), columns [c_lo, c_hi) (0 / 0:
 * all; other columns of g are not written); frames >= a clip's length receive 0.  g must not alias z. */
int dsh_op_guidance_grad(void* hip_stream, const float* z, float* g, int32_t B, int32_t frames, int32_t channels, int32_t c_lo, int32_t c_hi,
                         const dsh_guide* guide);
/* The guided form of dsh_op_ddim_step_full (second_order = 0) and of dsh_op_dpm2m_step (second_order != 0; x0_out is the history), one pass
 * in place: x0 = c1 x - c2 eps (clamped when clip), e = (c1 x - x0) / c2, e' = e - sqrt_1m_ab g, x0' = c1 x - c2 e', then the parent's
 * update from x0' (x0_out receives x0').  g is taken on x (DSH_GUIDE_XT) or on x0 (DSH_GUIDE_X0: the neighbouring frames' x0 are
 * re-derived from their x and eps).  An element whose g is exactly 0 takes the parent's update bit for bit.  Columns outside
 * [c_lo, c_hi) and frames >= a clip's length are not touched.  No saved noisy tails in this entry. */
int dsh_op_guided_ddim_step(void* hip_stream, float* x, const float* eps, float* x0_out, const float* gt, const uint8_t* mask, const float* noise2,
                            const float* noise1, const dsh_guide* guide, int32_t B, int32_t frames, int32_t channels, float c1, float c2,
                            float sqrt_ab_prev, float sqrt_1m_ab_prev, float coef_eps, float sigma, float sqrt_1m_ab, float A, float Bc, float G,
                            int32_t second_order, int32_t overlap_len, int32_t blend, int32_t tail_blend, int32_t clip, int32_t c_lo, int32_t c_hi);
/* The guided form of dsh_op_ddpm_step on x [B, frames, channels]: mean' = mean + post_var g (condition_mean), otherwise as the parent. */
int dsh_op_guided_ddpm_step(void* hip_stream, float* x, const float* eps, const float* noise, float* x0_out, const dsh_guide* guide, int32_t B,
                            int32_t frames, int32_t channels, float c1, float c2, float coef1, float coef2, float sigma, float post_var,
                            int32_t clip, int32_t c_lo, int32_t c_hi);
/* x <- sqrt_1m_beta x + sqrt_beta noise; a channel range needs the channel count. */
int dsh_op_undo_step(void* hip_stream, float* x, const float* noise, float sqrt_1m_beta, float sqrt_beta, int64_t n, int32_t channels,
                     int32_t c_lo, int32_t c_hi);
/* Timestep-cache copy: nseg <= 4 byte ranges (host arrays: device pointers work_dev[i], bytes[i], off[i]; multiples of 16) between the work
 * buffers and slots + *level_dev * stride + off[i]; restore 0 saves, 1 restores.  Refuses a range that leaves its slot. */
int dsh_op_level_copy(void* hip_stream, void* const* work_dev, const int64_t* bytes, const int64_t* off, int32_t nseg, void* slots, int64_t stride,
                      const int64_t* level_dev, int32_t restore);
/* t[0, n) = tv, c1[0, n) = c1v, c2[0, n) = c2v, *level = lv in one launch. */
int dsh_op_fill_step(void* hip_stream, int64_t* t, float* c1, float* c2, int64_t* level, int64_t tv, float c1v, float c2v, int64_t lv, int32_t n);
/* p[0, n) = host[0, n) in stream order (64 values per launch travel as kernel arguments). */
int dsh_op_store_values_f32(void* hip_stream, float* p, const float* host, int32_t n);
/* x[b, t, :] = 0 for t >= lens_dev[b]; x [B, frames, channels]. */
int dsh_op_zero_padded_frames(void* hip_stream, float* x, const int32_t* lens_dev, int32_t B, int32_t frames, int32_t channels);
/* columns [c_lo, c_hi) of dst [M, C] <- the first c_hi - c_lo columns of src [M, src_ld], or 0 when src is NULL. */
int dsh_op_fill_cols(void* hip_stream, float* dst, int32_t C, int64_t M, int32_t c_lo, int32_t c_hi, const float* src, int32_t src_ld);
/* timestep_embedding (models/transformer.py:42-59): out[b, :dim] = (cos(t_b f_j) | sin(t_b f_j)), f_j = exp(-ln(1e4) j / (dim / 2)) in fp32;
 * t_dev int64 [B]; dtype 0: fp32 out, 1: bf16 out (uint16 bits); ldo >= dim. */
int dsh_op_temb(void* hip_stream, int32_t dtype, const int64_t* t_dev, int32_t B, int32_t dim, void* out, int32_t ldo);
/* classifier-free mix: eps[r, c0 + c] = u + s_b (k - u), u = o[r, c], k = o[r + cond_row0, c], s_b = scale[b * scale_row], b = r / frames
 * (s_b == 1: k itself; has_null == 0: a copy of o[r, c]), r < Mc, c < w; x0 (nullable) [Mc, ldx0] = c1[b] x[r, c0 + c] - c2[b] eps. */
int dsh_op_cfg_mix(void* hip_stream, const float* o, int32_t ldo, int32_t Mc, int32_t cond_row0, int32_t frames, int32_t w, int32_t has_null,
                   const float* scale, int32_t scale_row, float* eps, int32_t lde, int32_t c0, const float* x, int32_t ldx, const float* c1,
                   const float* c2, float* x0, int32_t ldx0);
/* the same under a guidance schedule (dsh_set_guidance_schedule states the formulas): the arguments of dsh_op_cfg_mix, then t (device int64,
 * clip b's model timestep t[b * t_row], clamped into the table), table (device fp32 [2, n_steps]), which (the row read), rescale (phi of
 * that row: 0 = one launch, > 0 = two, then the row moments live in scratch the entry owns) and lens_dev (device int32 [Mc / frames],
 * nullable = frames).  has_null == 0: dsh_op_cfg_mix itself.  Synchronises the stream. */
int dsh_op_cfg_mix_sched(void* hip_stream, const float* o, int32_t ldo, int32_t Mc, int32_t cond_row0, int32_t frames, int32_t w, int32_t has_null,
                         const float* scale, int32_t scale_row, float* eps, int32_t lde, int32_t c0, const float* x, int32_t ldx, const float* c1,
                         const float* c2, float* x0, int32_t ldx0, const int64_t* t, int32_t t_row, const float* table, int32_t n_steps,
                         int32_t which, float rescale, const int32_t* lens_dev);
/* Conv1d(k = 3, padding = 1) patches: out[(b, t), tap * Cin + c] = x[b, t + tap - 1, c], zero outside [0, len_b); lens_dev nullable (len_b =
 * frames).  dtype 0 fp32 / 1 bf16: fp32 -> fp32, fp32 -> bf16, bf16 -> bf16. */
int dsh_op_im2col3(void* hip_stream, int32_t dtype_in, int32_t dtype_out, const void* x, int32_t ldx, int32_t B, int32_t frames, int32_t Cin,
                   void* out, int32_t ldo, const int32_t* lens_dev);
/* FiLM rows [scale(D) | shift(D)] x nblk per clip -> [A | B], A = gamma (1 + scale), B = beta (1 + scale) + shift; gamma / beta [nblk, D].
 * film_fold: in place on tab [B, ld].  film_expand: dst[b] = fold(src[idx_dev[b]]) (idx_dev NULL: identity; fold 0: plain copy); D % 4 == 0. */
int dsh_op_film_fold(void* hip_stream, float* tab, int32_t ld, int32_t B, int32_t nblk, int32_t D, const float* gamma, const float* beta);
int dsh_op_film_expand(void* hip_stream, const float* src, int32_t ld, const int32_t* idx_dev, float* dst, int32_t B, int32_t nblk, int32_t D,
                       const float* gamma, const float* beta, int32_t fold);
/* dst[b, :w] = src[idx_dev[b], :w]. */
int dsh_op_gather_rows(void* hip_stream, const float* src, int32_t ld, const int32_t* idx_dev, float* dst, int32_t ldd, int32_t B, int32_t w);
/* Layer-0 seed of the residual stream from h0 [Mc, D]: rows [0, Mc) = h0 + c (has_null) or h0, rows [row1, row1 + Mc) = h0 (has_null; row1 a
 * multiple of 32, >= Mc).  Outputs row-major [R, D], R = (has_null ? row1 : 0) + round_up(Mc, 32); rows the kernel does not write come back
 * as 0.  hilo 0: h_out fp32 and h16_out = bf16(h); hilo 1: h16_out = hi plane, lo_out = bf16(h - hi), h_out untouched.  Synchronises. */
int dsh_op_seed_stream(void* hip_stream, const float* h0, int32_t Mc, int32_t D, const float* c, int32_t has_null, int32_t row1, int32_t hilo,
                       float* h_out, void* h16_out, void* lo_out);
/* Given expression track src [B frames, E] -> x0 [B frames, ld] (pad columns zero; frames >= lens_dev[b] zero) and, x16_out != NULL, the bf16
 * operand [B frames, 128] read back row-major; tiler_out (nullable, same shape): the library's bf16 tiler applied to the x0 rows just
 * written, which x16_out is documented to equal bit for bit.  E <= ld <= 128.  Synchronises. */
int dsh_op_pack_expr_track(void* hip_stream, const float* src, int32_t E, int32_t B, int32_t frames, const int32_t* lens_dev, float* x0, int32_t ld,
                           void* x16_out, void* tiler_out);
/* ln_rows with its constant fold: h[r] += pre_add for r < n_pre_rows (h in/out; pre_add nullable), out = LayerNorm(h) gamma + beta;
 * dtype 0 fp32 / 1 bf16 output. */
int dsh_op_layernorm_pre(void* hip_stream, int32_t dtype, float* h, int32_t ldh, int32_t M, int32_t D, const float* pre_add, int32_t n_pre_rows,
                         const float* gamma, const float* beta, void* out, int32_t ldo);
/* StylizationBlock front on rows: out = SiLU(LN(y) (1 + scale) + shift), (scale | shift) = film[(r / frames) % bmod, film_off ..];
 * variant 0: fp32 -> fp32, 1: fp32 -> bf16, 2: bf16 -> bf16. */
int dsh_op_ln_film_silu(void* hip_stream, int32_t variant, const void* y, int32_t ldy, int32_t M, int32_t D, const float* gamma, const float* beta,
                        const float* film, int32_t film_ld, int32_t film_off, int32_t frames, int32_t bmod, void* out, int32_t ldo);
/* LayerNorm over the virtual concat row [p0 (fp32, w0) | p1 (w1) | p2 (w2) | p3 (fp32, w3, may be 0)]; p1 / p2 and out have the element type
 * of dtype (0 fp32 / 1 bf16); columns [P, Ppad) of out are written as zero. */
int dsh_op_concat_ln(void* hip_stream, int32_t dtype, const float* p0, int32_t ld0, int32_t w0, const void* p1, int32_t ld1, int32_t w1,
                     const void* p2, int32_t ld2, int32_t w2, const float* p3, int32_t ld3, int32_t w3, int32_t M, const float* gamma,
                     const float* beta, void* out, int32_t ldo, int32_t Ppad);

/* ---- validation metrics (trainers/ddpm_show_trainer.py:440-583, ddpm_beat_trainer.py:489-644) ------------------------- */
/* The FGD pose encoder: HalfEmbeddingNet.forward = PoseEncoderConv in eval() mode (models/motion_autoencoder.py:38-100, 192-204), fp32 on
 * the exact-fp32 matrix pipe.  A handle of its own, independent of a dsh_ctx context (an eval model is another network with other weights), bound
 * to one (device, stream), not thread-safe.  n_poses = frames per clip the network is built for (88, 64 and 34 have an out_net in the
 * reference; every other length is built like 88 / 64: four Linears behind the flatten), dim = channels per frame (any width),
 * vae_length = the reference's `base` (300), a multiple of 4.  hip_stream as for dsh_create (NULL: a stream of its own).  No device is
 * touched before dsh_fgd_finalize. */
typedef struct dsh_fgd dsh_fgd;
int dsh_fgd_create(int32_t n_poses, int32_t dim, int32_t vae_length, void* hip_stream, dsh_fgd** out);
int dsh_fgd_destroy(dsh_fgd* h);
/* Weights by the state-dict key names of HalfEmbeddingNet (fp32 host memory, copied): pose_encoder.net.{0,1,2}.0.{weight,bias} (Conv1d
 * [out, in, k]), pose_encoder.net.{0,1,2}.1.{weight,bias,running_mean,running_var} (BatchNorm1d), pose_encoder.net.3.{weight,bias},
 * pose_encoder.out_net.<i>.* (Linears and BatchNorms at the reference's indices), pose_encoder.fc_mu.{weight,bias}.  decoder.*,
 * pose_encoder.fc_logvar.* and *.num_batches_tracked are accepted and ignored (the reference loads them and forward() never uses them).
 * -1 on an unknown key or a shape other than the network's. */
int dsh_fgd_load_tensor(dsh_fgd* h, const char* name, const float* host_data, const int64_t* shape, int32_t ndim);
/* Builds the device layout: eval-mode BatchNorm folded into the conv / Linear in front of it (fp64), conv weights repacked to
 * [out, k * in] (tap-major, channel minor: the implicit-GEMM row of channels-last activations), the first Linear's columns permuted from
 * the reference's channel-major flatten (c * frames + t) to channels-last (t * vae_length + c), every K padded with zeros to 32 floats.
 * -1 naming the first missing key. */
int dsh_fgd_finalize(dsh_fgd* h);
/* Test helper, host only (runs without a GPU): layer `index` exactly as dsh_fgd_finalize would upload it, once every tensor is loaded and
 * before dsh_fgd_finalize (which releases the staged copies).  Layers 0 .. 3 are the convolutions, then the out_net Linears, fc_mu last
 * (dsh_fgd_debug_num_layers).  dims3 = {N, K, K padded}; W [N, K padded] and bias [N] are nullable host buffers. */
int32_t dsh_fgd_debug_num_layers(const dsh_fgd* h);
int dsh_fgd_debug_packed_layer(const dsh_fgd* h, int32_t index, int32_t* dims3, float* W, float* bias);
/* latents[B, vae_length] = mu(x[:, :n_poses, :]) for x [B, frames, dim] (device fp32), frames >= n_poses: only the first n_poses frames
 * of each clip are read (outputs[:, :88, :] in the reference), whatever the rest holds.  Asynchronous on the handle's stream; -1 (nothing
 * launched) when frames < n_poses.  A larger batch than any before grows the handle's buffers, which waits for the stream once. */
int dsh_fgd_encode(dsh_fgd* h, const float* x, int32_t batch, int32_t frames, float* latents);
/* Test helper: ONE launch of the encoder's implicit-GEMM Conv1d (conv_gemm_f32_kernel) on hip_stream, no scratch, nothing synchronises:
 *   Y[b * y_clip + t * N + n] = act(bias[n] + sum_{k < Kreal} X[b * x_clip + t * x_step + k] * W[n * ldw + k]),  b < B, t < Tout, n < N,
 * act = LeakyReLU(0.2) when leaky, the identity otherwise.  For a Conv1d (kernel ksize, stride s) over channels-last clips [Tin, Cin]:
 * x_step = s * Cin, Kreal = ksize * Cin, Tout = (Tin - ksize) / s + 1, W = [N, (tap, channel)].  Kp = Kreal rounded up to 32 floats, the
 * weights zero padded to it (ldw >= Kp); on the activation side only the Kreal floats of a row are read.  All device fp32, 16-byte aligned;
 * Kreal, x_step, x_clip, ldw, N and y_clip are multiples of 4.  -1 (nothing launched) otherwise. */
int dsh_op_conv_gemm_f32(void* hip_stream, const float* X, int64_t x_clip, int32_t x_step, const float* W, int32_t ldw, const float* bias, float* Y,
                         int64_t y_clip, int32_t B, int32_t Tout, int32_t N, int32_t Kreal, int32_t Kp, int32_t leaky);

/* MSE, PCK and diversity of one validation batch (ddpm_show_trainer.py:516-550) from outputs / motions [B, T, C] (device fp32) in three
 * launches on hip_stream; nothing synchronises, fixed-order reductions (two runs: identical bits).
 *   diff = outputs - motions;  MSE = mean(diff^2) (fp64 accumulation);
 *   PCK  = mean over the B T C / joint_dim joints of [sqrt(sum_j diff_j^2) < 0.5], fp32 as numpy computes it: joint_dim 1 = per element
 *          (SHOW: unsqueeze(-1)), 3 = per consecutive channel triplet (BEAT: reshape(B, T, C / 3, 3)); C % joint_dim == 0;
 *   diversity of group g (clips [g b_div, (g + 1) b_div), g < B / b_div: the incomplete last group is dropped, as in the reference)
 *          = 2 / (b_div (b_div - 1)) * sum_{i<j} mean_e |o_i[e] - o_j[e]|.  The reference uses b_div = min(50, B); 2 <= b_div <= min(B, 128).
 * result_dev: device buffer of dsh_batch_metrics_result_bytes(B, T, C, b_div) bytes, 8-byte aligned, 8-byte words:
 *   [0] double  sum diff^2          [1] int64  PCK count (joints below 0.5)      [2] double MSE       [3] double PCK
 *   [4] int64   groups = B / b_div  [5 .. 5 + groups) double diversity per group;   everything behind is scratch (block partials). */
#define DSH_METRICS_HEADER 5
int64_t dsh_batch_metrics_result_bytes(int32_t B, int32_t T, int32_t C, int32_t b_div);
int dsh_op_batch_metrics(void* hip_stream, const float* outputs, const float* motions, int32_t B, int32_t T, int32_t C, int32_t joint_dim,
                         int32_t b_div, void* result_dev);

/* The loss terms of the reference's eval-mode training forward (GaussianDiffusion.training_losses, gaussian_diffusion.py:1319-1426, epsilon / MSE
 * branch; backward_G, ddpm_beat_trainer.py:222-260) from eps (the model output), noise, x_t and x0 [B, T, C] (device fp32, 4-byte aligned) in two
 * launches on hip_stream; nothing synchronises, fixed-order reductions (two runs: identical bits; a row's numbers do not depend on B or on its
 * position in the batch).  c1_dev / c2_dev: device arrays [B], sqrt_recip_alphas_cumprod[t_b] / sqrt_recipm1_alphas_cumprod[t_b].
 *   x0_pred = c1 x_t - c2 eps, products and difference rounded on their own: the bits dsh_op_ddim_step_full writes to x0_out.
 * lens_dev (DEVICE int32 [B], nullable, clamped to [0, T]): row b owns its first lens_dev[b] frames; no frame behind is read, frame pairs
 * (f, f + 1) exist for f < lens[b] - 1.  split: the gesture | expression column boundary, 0 < split < C.  C <= 448.  Differences and
 * quotients are single fp32 operations, squares and sums fp64.  Optional outputs (nullable): x0_pred_out [B, T, C] and frame_mse_out [B, T]
 * = mean over C of (eps - noise)^2 per frame; both 0 on frames >= lens[b].
 * result_dev: device buffer of dsh_denoise_losses_result_bytes(B, T) bytes, 8-byte aligned, doubles:
 *   [0] loss_model_pred = 1000 * sum over valid frames of frame_mse / valid frames   [1] loss_vel_rec = 100 * V, V = the same mean over the
 *   valid frame pairs of mean_C of term 3   [2] loss_x0_rec = 100 * huber_beta * mean over valid elements of term 4
 *   [3] final_loss = [0] + V + [2] (the reference adds the UNSCALED velocity term, ddpm_beat_trainer.py:247)
 *   [4] valid frames  [5] valid frame pairs  [6] valid elements  [7] 0;  a mean over a zero count is written as 0
 *   [8 + 7 b + j] row b, term j:  0 sum (eps - noise)^2 over columns < split   1 the same over columns >= split   2 sum (x0_pred - x0)^2
 *     3 sum over pairs of ((x0_pred[f] - x0_pred[f + 1]) - (x0[f] - x0[f + 1]))^2   4 sum smooth_l1(x0 / huber_beta, x0_pred / huber_beta)
 *     at threshold 1   5 lens[b] * C   6 lens[b] - 1;   everything behind the rows is scratch (block partials).
 * -1 (nothing launched) on a null pointer, a non-positive dim, split outside (0, C), huber_beta <= 0 or a misaligned pointer. */
#define DSH_LOSS_HEADER 8
#define DSH_LOSS_COLS 7
int64_t dsh_denoise_losses_result_bytes(int32_t B, int32_t T);
int dsh_op_denoise_losses(void* hip_stream, const float* eps, const float* noise, const float* x_t, const float* x0, const float* c1_dev,
                          const float* c2_dev, const int32_t* lens_dev, int32_t B, int32_t T, int32_t C, int32_t split, float huber_beta,
                          float* x0_pred_out, float* frame_mse_out, void* result_dev);

/* ---- audio front (trainers/ddpm_show_trainer.py:944-1100, test_custom_aud) -------------------------------------------------- */
/* The mel spectrogram test_custom_aud computes: librosa.feature.melspectrogram(y, sr, hop_length = hop, n_mels)[..., :-1] (power 2, no
 * logarithm, center = True with reflect padding, periodic Hann window of n_fft samples, Slaney filterbank from 0 to sr / 2 with Slaney
 * normalisation), fp32 on the exact-fp32 matrix pipe.  The reference's call is (18000, 2048, 1200, 128).  A handle of its own, bound to one
 * (device, stream), not thread-safe; hip_stream as for dsh_create (NULL: a stream of its own).  n_fft a multiple of 32, hop and n_mels
 * multiples of 4.  Creating the handle builds two tables on the host in fp64 and stores them as fp32; no device is touched before the first
 * dsh_mel_compute.
 *   dft [2 (n_fft / 2 + 1), n_fft]   row k = w[i] cos(2 pi k i / n_fft), row n_fft / 2 + 1 + k = w[i] sin(2 pi k i / n_fft),
 *                                    w[i] = 0.5 - 0.5 cos(2 pi i / n_fft); the angle is reduced exactly, (k i) mod n_fft, before cos / sin
 *   fb  [n_mels, n_fft / 2 + 1]      mel(f) = 3 f / 200 below 1000 Hz, 15 + 27 ln(f / 1000) / ln 6.4 above; n_mels + 2 points m_i equally
 *                                    spaced in mel from 0 to sr / 2; fb[i, k] = max(0, min((f_k - m_i) / (m_{i+1} - m_i),
 *                                    (m_{i+2} - f_k) / (m_{i+2} - m_{i+1}))) * 2 / (m_{i+2} - m_i) at f_k = k sr / n_fft */
typedef struct dsh_mel dsh_mel;
int dsh_mel_create(int32_t sr, int32_t n_fft, int32_t hop, int32_t n_mels, void* hip_stream, dsh_mel** out);
int dsh_mel_destroy(dsh_mel* h);
/* Frames of a signal of len samples: len / hop (of the 1 + len / hop centred frames the reference drops the last), or -1 when
 * len < n_fft / 2 + 1 (the reflect padding needs that many samples) or len < hop (no frame). */
int64_t dsh_mel_num_frames(const dsh_mel* h, int64_t len);
/* Test helper, host only (runs without a GPU): dims3 = {n_fft / 2 + 1, n_fft, n_mels} and the two tables above (nullable host buffers). */
int dsh_mel_debug_tables(const dsh_mel* h, int32_t* dims3, float* dft, float* fb);
/* mel[B, N, n_mels] (N = dsh_mel_num_frames(len)) from wave [B, len], both device fp32, mel 16-byte aligned.  Frame j is samples
 * [hop j - n_fft / 2, hop j + n_fft / 2) of the reflect-padded signal.  Four launches on the handle's stream, asynchronous: reflect padding,
 * the windowed DFT as an implicit GEMM over overlapping rows (K = n_fft), the power spectrum re^2 + im^2, the filterbank GEMM.  Fixed
 * summation order; a row's result does not depend on B; a silent input gives exact zeros.  -1 (nothing launched) when dsh_mel_num_frames
 * is -1, on a null pointer or B < 1.  A larger B x len than any before grows the handle's buffers, which waits for the stream once. */
int dsh_mel_compute(dsh_mel* h, const float* wave, int32_t batch, int64_t len, float* mel);
/* Utterances of different lengths in one call: wave [B, len] padded, row b owning lens_dev[b] samples (DEVICE int32 [B]; the caller has checked
 * dsh_mel_num_frames(lens[b]) >= 1 and lens[b] <= len: a count outside gives a row of zeros).  mel [B, dsh_mel_num_frames(len), n_mels]; its
 * frames j < lens[b] / hop are bit for bit what dsh_mel_compute gives for row b alone at len = lens[b] (the reflection is about the row's own last
 * sample; the GEMMs run on the padded rows), the frames behind are 0.  No sample behind lens[b] is read, so the padding may hold anything.  One
 * launch more than the dense call.  -1 as dsh_mel_compute, and on null lengths. */
int dsh_mel_compute_ragged(dsh_mel* h, const float* wave, int32_t batch, int64_t len, const int32_t* lens_dev, float* mel);

/* scipy.signal.resample_poly(x, up, down, window = taps / up) for caller-supplied FIR taps (an odd number, gain included, DEVICE fp32):
 * zero-stuff by up, filter, decimate by down, the taps centred, zeros outside the signal:
 *   y[b, j] = sum_k taps[k] x[b, (j down + (n_taps - 1) / 2 - k) / up]  over the k for which the index is an integer in [0, n), k ascending,
 * for j < dsh_resample_poly_len(n, up, down) = ceil(n up / down).  up / down are used as given (reduce them by their gcd first, as scipy
 * does).  x [B, n], y [B, n_out] device fp32.  One lane per output sample, about n_taps / up products each. */
int64_t dsh_resample_poly_len(int64_t n, int32_t up, int32_t down);
int dsh_op_resample_poly(void* hip_stream, const float* x, int32_t batch, int64_t n, int32_t up, int32_t down, const float* taps_dev, int32_t n_taps,
                         float* y);

/* x [B, n] padded, row b owning lens_dev[b] samples (DEVICE int32 [B], clamped to [0, n]): y [B, dsh_resample_poly_len(n)], row b what
 * dsh_op_resample_poly gives for its own samples alone (the taps at the right edge see nothing behind lens[b]), 0 behind
 * dsh_resample_poly_len(lens[b]).  No sample behind lens[b] is read. */
int dsh_op_resample_poly_ragged(void* hip_stream, const float* x, int32_t batch, int64_t n, const int32_t* lens_dev, int32_t up, int32_t down,
                                const float* taps_dev, int32_t n_taps, float* y);

/* Softmax multi-head attention core with 64-wide heads and no mask, fp32 on the exact-fp32 matrix pipe:
 *   out[b, t, 64 h + d] = sum_s softmax_s(q[b, t, h] . k[b, s, h]) v[b, s, 64 h + d],   qkv [B, M, 3 H 64] = (q | k | v) per row, q already
 * scaled; out [B, M, H 64]; both device fp32, 16-byte aligned.  One wave per (b, h, 32 queries), keys in tiles of 32 with an online maximum
 * and sum (logits of any size), keys >= M of the last tile weigh exactly 0.  Fixed order: row b does not depend on B. */
int dsh_op_softmax_attention(void* hip_stream, const float* qkv, int32_t B, int32_t M, int32_t H, float* out);
/* The same kernel body for rows of M_max frames of which row b owns lens_dev[b] (DEVICE int32 [B], clamped to [0, M_max]): queries and keys
 * < lens[b] only, the loads, products and exponentials of the dense call on row b alone at M = lens[b] in the same order, hence the same bits;
 * out[b, t >= lens[b]] = 0.  No frame >= lens[b] is read (a NaN there would survive a zero weight); query tiles behind lens[b] do no matrix
 * work. */
int dsh_op_softmax_attention_ragged(void* hip_stream, const float* qkv, int32_t B, int32_t M_max, int32_t H, const int32_t* lens_dev, float* out);

/* The HuBERT encoder of the hubert-large family (transformers' HubertModel with feat_extract_norm = "layer", conv_bias = True,
 * do_stable_layer_norm = True, feat_proj_layer_norm = True), fp32 on the exact-fp32 matrix pipe: the `pretrain_aud_feat` test_custom_aud computes
 * from a 16 kHz signal.  A handle of its own, bound to one (device, stream), not thread-safe; hip_stream as for dsh_create.  No device is
 * touched before dsh_hubert_finalize.  Supported (dsh_hubert_create gives -1 otherwise, before any device work): hidden / heads == 64,
 * hidden <= 1024, every conv_dim a multiple of 32 (at most 1024), (hidden / pos_groups) % 32 == 0, pos_kernel even, hidden and intermediate
 * multiples of 32, ln_eps == 1e-5 (the folded-LayerNorm launch has that value built in).  hubert-large: hidden 1024, 24 layers, 16 heads,
 * intermediate 4096, conv_dim 512 x 7, conv_kernel (10, 3, 3, 3, 3, 2, 2), conv_stride (5, 2, 2, 2, 2, 2, 2), pos_kernel 128, pos_groups 16. */
typedef struct dsh_hubert_config {
    int32_t hidden, layers, heads, intermediate;
    int32_t conv_dim[7], conv_kernel[7], conv_stride[7];
    int32_t pos_kernel, pos_groups;
    float ln_eps;
} dsh_hubert_config;
typedef struct dsh_hubert dsh_hubert;
int dsh_hubert_create(const dsh_hubert_config* cfg, void* hip_stream, dsh_hubert** out);
int dsh_hubert_destroy(dsh_hubert* h);
/* Weights by the state-dict keys of HubertModel (fp32 host memory, copied):
 *   feature_extractor.conv_layers.{i}.conv.{weight [out, in, k], bias}, .layer_norm.{weight, bias}           i = 0 .. 6 (in = 1 for i = 0)
 *   feature_projection.layer_norm.{weight, bias}, feature_projection.projection.{weight [hidden, conv_dim[6]], bias}
 *   encoder.pos_conv_embed.conv.bias and the weight-norm pair, in either spelling: conv.weight_g [1, 1, k] / conv.weight_v
 *   [hidden, hidden / groups, k] (transformers 4.31) or conv.parametrizations.weight.original0 / original1 (current)
 *   encoder.layers.{l}.attention.{q,k,v,out}_proj.{weight, bias}, .layer_norm.*, .feed_forward.{intermediate_dense, output_dense}.*,
 *   .final_layer_norm.*;  encoder.layer_norm.{weight, bias}
 * masked_spec_embed and lm_head.* are accepted and ignored.  -1 on an unknown key or a shape other than the configuration's. */
int dsh_hubert_load_tensor(dsh_hubert* h, const char* name, const float* host_data, const int64_t* shape, int32_t ndim);
/* Builds the device layout in fp64 on the host: the positional conv weight w[o, i, k] = g[k] v[o, i, k] / |v[:, :, k]|_2 (norm over (o, i) per
 * tap); conv weights repacked to [out, k * in], tap-major; each layer's first LayerNorm folded into ONE q|k|v weight [3 hidden, hidden] whose q
 * rows (weight and bias) carry the 1 / 8 of the 64-wide heads; final_layer_norm folded into intermediate_dense; the feature projection's
 * LayerNorm folded into the projection.  Folds in the pro 1 convention of dsh_op_gemm_f32_pro: W' = gamma (.) W, b' = b + W beta, fc = row sums
 * of W' as rounded to fp32.  -1 naming the first missing key. */
int dsh_hubert_finalize(dsh_hubert* h);
/* Test helper, host only (runs without a GPU), before dsh_hubert_finalize: one Linear / convolution as it would be uploaded.  kind 0: conv
 * `layer` (0 .. 6), 1: feature projection, 2: positional conv ([hidden, k * hidden / groups], tap-major), 3: q|k|v of `layer`, 4: out_proj,
 * 5: intermediate_dense, 6: output_dense.  dims2 = {N, K}; W [N, K], bias [N], fc [N] (zeros for the kinds without a fold); all nullable. */
int dsh_hubert_debug_packed(const dsh_hubert* h, int32_t kind, int32_t layer, int32_t* dims2, float* W, float* bias, float* fc);
/* Frames of n samples: L_i = (L_{i-1} - k_i) / s_i + 1 through the seven convolutions ((n - 400) / 320 + 1 at the large strides), or -1 when n is
 * shorter than the receptive field (400). */
int64_t dsh_hubert_num_frames(const dsh_hubert* h, int64_t n);
/* Batch rows the convolution stack processes per pass (default 4; its activations are 131 MB per 20 s row at the large widths).  The pass size
 * never changes a bit of the result. */
int dsh_hubert_set_chunk_pass(dsh_hubert* h, int32_t rows);
/* out[B, M, hidden] (M = dsh_hubert_num_frames(n)) = last_hidden_state of x [B, n], a signal the caller has already normalised (zero mean,
 * unit variance over the utterance); both device fp32, out 16-byte aligned.  Asynchronous on the handle's stream.  Every reduction has a fixed
 * order and there are no atomics: row b has the same bits whatever B and the pass size are.  -1 (nothing launched) when n is shorter than the
 * receptive field, on a null pointer or B < 1.  A larger B x n than any before grows the handle's buffers, which waits for the stream once. */
int dsh_hubert_encode(dsh_hubert* h, const float* x, int32_t batch, int64_t n, float* out);
/* Utterances of different lengths in one call: x [B, n_max] padded, row b owning lens_samples[b] samples (HOST int64 [B]).  out [B, M_max, hidden],
 * M_max = dsh_hubert_num_frames(n_max); frames t < dsh_hubert_num_frames(lens_samples[b]) of row b are bit for bit dsh_hubert_encode of that row
 * alone at n = lens_samples[b], whatever the samples behind hold (NaN included), the frames behind are 0.  The convolution stack and the Linears
 * run on the padded rows (a valid convolution's frame t < M_b reads samples < n_b only); the positional convolution, the attention and the last
 * LayerNorm take the frame counts, uploaded once per call (which waits for the handle's stream).  -1 (nothing launched, out untouched) for a row
 * shorter than the receptive field, lens_samples[b] > n_max, null lengths, and as dsh_hubert_encode. */
int dsh_hubert_encode_ragged(dsh_hubert* h, const float* x, int32_t batch, int64_t n_max, const int64_t* lens_samples, float* out);
/* Precision of the transformer layers: 0 = fp32 (the default, bit for bit what it was), 1 = bf16.  Only before dsh_hubert_finalize (-1 with a
 * dsh_last_error text afterwards, and for any other value, or when hidden or intermediate is not a multiple of 64).
 * bf16: the convolution stack, the feature projection, the positional convolution and the last LayerNorm stay the fp32 launches, so the
 * residual stream h behind the positional convolution has the bits of the fp32 encoder; h stays fp32 in memory throughout.  Per layer
 *   W' = RNE_bf16(gamma (.) W) rounded once from the fp64 fold (q rows x 1 / 8 first, exact), b' = fp32(b + W beta); no fc vector;
 *   LayerNorm in front of q|k|v and intermediate_dense: two-pass fp32 (mean, rstd) per row (one small launch), a = RNE_bf16((h - mean) rstd)
 *   formed while the A operand is staged (no normalised copy in memory);
 *   q|k|v: fp32 accumulation + bias, RNE bf16 store; attention as dsh_op_softmax_attention_bf16; out_proj: h += acc + bias in fp32, in place;
 *   intermediate_dense: erf-GELU in fp32 on acc + bias, RNE bf16 store; output_dense: h += acc + bias in fp32, in place.
 * One accumulator with K ascending per output element, no split-K, no atomics: the bit identities of dsh_hubert_encode[_ragged] hold.
 * The layers' fp32 weights are not uploaded (hubert-large: about 0.6 GB of weights on the device instead of 1.26 GB).  Outputs stay fp32.
 * dsh_hubert_debug_packed then returns, for kinds 3 .. 6, W as fp32 values that are exactly the bf16-rounded weights and fc = 0. */
int dsh_hubert_set_precision(dsh_hubert* h, int32_t precision);
/* Test tap: every following encode call copies h [B M, hidden] as the positional convolution leaves it to h_posconv_dev (device fp32, on the
 * handle's stream); null switches it off. */
int dsh_hubert_debug_tap(dsh_hubert* h, float* h_posconv_dev);
/* Linear of the bf16 layers on v_mfma_f32_32x32x16_bf16 (gemm_bf16_pro.hip): C = act(pro(A) W^T + bias) (+ R), M >= 1, K % 64 == 0, N % 64 == 0
 * (-1 before any launch otherwise).  a_f32 = 1: A fp32 [M, K], staged as RNE_bf16((x - mean) rstd) with mom [M] (mean, rstd) pairs, or, mom null,
 * with the rows' own two-pass moments (eps 1e-5, K <= 1024) computed into per-call scratch; a_f32 = 0: A bf16 [M, K], staged as it is.  W bf16 bits
 * in natural [N, K] order (the kernel's packed order is that order).  bias fp32 [N].  act 0 or 2 (erf-GELU, on acc + bias).  R: fp32 residual [M, N]
 * or null, may be Cf.  Exactly one of Cf (fp32) and Cb (RNE bf16), [M, N]; R needs Cf.  tile 0: the launcher picks, 1 / 2: 64 x 64 / 128 x 128
 * (same bits).  One accumulator per output with K ascending. */
int dsh_op_gemm_bf16_pro(void* hip_stream, const void* A, int32_t a_f32, const float* mom, const void* W, const float* bias, const float* R,
                         float* Cf, void* Cb, int32_t M, int32_t N, int32_t K, int32_t act, int32_t tile);
/* dsh_op_softmax_attention[_ragged] on bf16 operands: qkv [B, M, 3 H 64] and out [B, M, H 64] device bf16, 16-byte aligned.  fp32 logits from
 * the bf16 q^ and k^, online softmax in fp32, p = exp(s - m) in fp32 with the row sum l over the unrounded p and RNE_bf16(p) as the operand of
 * the second product, o = (sum p^ v) / l in fp32, RNE bf16 store.  Keys >= M (lens[b]) weigh exactly 0 and are never loaded; ragged rows have
 * the bits of the dense call on the row alone, zeros behind lens[b]. */
int dsh_op_softmax_attention_bf16(void* hip_stream, const void* qkv, int32_t B, int32_t M, int32_t H, void* out);
int dsh_op_softmax_attention_bf16_ragged(void* hip_stream, const void* qkv, int32_t B, int32_t M_max, int32_t H, const int32_t* lens_dev, void* out);
/* The encoder's new kernels on row-major operands (op tests).
 * dsh_op_pos_conv: out[b, t, o] = h[b, t, o] + GELU(bias[o] + sum_{tap, i} W[o, tap cg + i] h[b, t + tap - k / 2, g cg + i]), cg = hidden / groups,
 *   g = o / cg: Conv1d(hidden, hidden, k, padding k / 2, groups) with its last output frame dropped (k even); frames outside [0, M) count as
 *   zeros and are never loaded.  h, out [B, M, hidden] (not aliased), W [hidden, k cg].
 * dsh_op_conv0_ln_gelu: y [B, (n - k) / stride + 1, C] = GELU(LayerNorm_C(Conv1d(1, C, k, stride)(x [B, n]))), W [C, k].
 * dsh_op_conv_ln_gelu: the same for channels-last x [B, L, Cin] and W [Cout, k Cin] tap-major: implicit GEMM + a LayerNorm / GELU row pass. */
int dsh_op_pos_conv(void* hip_stream, const float* h, int32_t B, int32_t M, int32_t hidden, int32_t groups, int32_t pos_kernel, const float* W,
                    const float* bias, float* out);
/* dsh_op_pos_conv with frame counts per batch row (DEVICE int32 [B], clamped to [0, M_max]): frames t >= lens[b] count as zeros like the frames
 * outside [0, M) and are never loaded; out[b, t >= lens[b]] = 0; row b has the bits of dsh_op_pos_conv on it alone at M = lens[b]. */
int dsh_op_pos_conv_ragged(void* hip_stream, const float* h, int32_t B, int32_t M_max, int32_t hidden, int32_t groups, int32_t pos_kernel,
                           const float* W, const float* bias, const int32_t* lens_dev, float* out);
int dsh_op_conv0_ln_gelu(void* hip_stream, const float* x, int32_t B, int64_t n, int32_t C, int32_t k, int32_t stride, const float* W, const float* bias,
                         const float* gamma, const float* beta, float* y);
int dsh_op_conv_ln_gelu(void* hip_stream, const float* x, int32_t B, int32_t L, int32_t Cin, int32_t Cout, int32_t k, int32_t stride, const float* W,
                        const float* bias, const float* gamma, const float* beta, float* y);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSHEG_HIP_H */
