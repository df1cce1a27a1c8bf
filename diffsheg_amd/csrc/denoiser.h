// Device-side UniDiffuser denoiser (models/transformer.py:590-770) for one (device, stream).
#pragma once
#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "dsh_common.h"
#include "dsh_kernels.h"
#include "profiler.h"
#include "switches.h"

namespace dsh {

struct ModelConfig {
    int dim_pose = 129, expression_dim = 103, style_dim = 4;
    int classifier_free = 1;
    float cond_scale = 1.25f;      // the context's guidance scale until dsh_set_guidance_scale() changes it (capi.hip)
    int latent_dim = 512, ff_size = 1024, num_layers = 8, num_heads = 8;
    int audio_dim = 128, aud_latent_dim = 256, hubert_dim = 1024, hubert_enc_dim = 128;
    int precision = 0;   // 0 = fp32 (exact-fp32 MFMA), 1 = bf16 storage + bf16 MFMA, fp32 accumulate, 2 = fp32 storage with the large Linears on the
                         // split-bf16 main loop (gemm_f32_split.hip; everything else is precision 0's)
    bool fp32_storage() const { return precision == 0 || precision == 2; }
    bool split_linears() const { return precision == 2; }
    // 1: the model is ONE MotionTransformer over all dim_pose + expression_dim channels (runner.py:46-57, opt.unidiffuser =
    // False, model_base transformer_encoder): no encoder_aud, audio_proj on the 128 mel features, no expression -> gesture flow
    int single_transformer = 0;
    int diffusion_steps = 1000;    // length of the original timestep scale: what a guidance schedule has one gain per (dsh_set_guidance_schedule)
    int channels() const { return dim_pose + expression_dim; }
    int time_embed_dim() const { return 4 * latent_dim; }
};

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
    size_t numel() const { return data.size(); }
};

// Timestep-level cache.  In every sampling loop all rows of an evaluation share one timestep, and part of an evaluation
// does not depend on x at all: the time / speaker / FiLM embeddings, encoder_aud and audio_proj are functions of
// (condition, t) only (transformer.py:730-739, :555-559, :574).  Loops that revisit levels (the out-painting jump schedule:
// 63 evaluations over 16 levels) compute that part once per level.  The mode of eval_level(mode, level); slots die with the next set_condition():
enum EvalMode {
    EVAL_PLAIN = 0,      // the whole evaluation
    EVAL_SAVE = 1,       // ... and save the x-independent results into slot *level (device int64)
    EVAL_RESTORE = 2,    // restore them from slot *level instead of recomputing them
    EVAL_HEAD_ONLY = 3,  // compute and save the x-independent results only (no evaluation; x / c1 / c2 / eps may be null): what a second
};                       // instance on a side stream runs AHEAD of the loop
// what set_part() / set_modality() select: the whole (joint) evaluation, the expression encoder only, the gesture encoder only
enum Part { PART_BOTH = 0, PART_EXPRESSION = 1, PART_GESTURE = 2 };

// One model instance on one stream: weights (owned, or shared with the instance it was cloned from), workspace, one condition, one
// evaluation.  Type-erased; the implementation is templated on the storage type (float / bf16).
class DenoiserInstance {
  public:
    virtual ~DenoiserInstance() {}
    virtual int finalize(const std::map<std::string, HostTensor>& w) = 0;
    // 0 if a batch of B clips of T frames can be evaluated, else -1 with the limit in the error text.  set_condition() asks before it
    // touches any state or queues any launch, so a refused shape leaves the context exactly as it was.
    virtual int check_shape(int B, int T) const = 0;
    //   set_lengths(): what a per-stream instance reads — device int32 [its clips], owned by the context, null = all full; takes effect
    //   with the instance's next set_condition() / set_condition_light() (hubert_encoder and encoder_aud's attention depend on it).
    virtual int set_lengths(const int* lens_dev) = 0;
    // step-invariant conditioning: audio [B,T,128] fp32, person_id [B,S] fp32, hubert [B,T,1024] fp32 (device)
    virtual int set_condition(int B, int T, const float* audio, const float* person_id, const float* hubert) = 0;
    // helpers of the prefetch path: the part of set_condition() the x-independent head needs; the timestep cache's slots, lent to a second instance
    virtual int set_condition_light(int B, int T, const float* audio, const float* person_id) = 0;
    virtual int level_slots(char** slots, size_t* stride, int* n) = 0;
    virtual int adopt_level_slots(char* slots, size_t stride, int n) = 0;
    //   level_cache_prepare(n): slots for n levels of the CURRENT condition; 0 if available (small batches only), else -1
    virtual int level_cache_prepare(int n_levels) = 0;
    // eps[B,T,C] = model(x[B,T,C], t[B]) with c1/c2 [B] (device fp32) feeding the expression x0; mode: EvalMode
    virtual int eval_level(const float* x, const int64_t* t, const float* c1, const float* c2, float* eps, int mode, const int64_t* level) = 0;
    // Classifier-free guidance of the next evaluations (transformer.py:537, :586): eps = u + s_b (k - u) with s_b = scale[b * scale_row] for clip b
    // (device fp32, read by the mix kernels when they run: a captured graph follows the buffer's contents), scale_row 0 = one value for the batch.
    // doubled = evaluate the null half at all (classifier-free weights and some s_b != 1); a clip at exactly 1 in a doubled batch takes k.  Grows
    // the token-row workspace the first time a doubled batch is asked for.  The scale buffer must outlive every evaluation that reads it.
    virtual int set_guidance(const float* scale, int scale_row, bool doubled) = 0;
    // Guidance schedule of the next evaluations (dsh_set_guidance_schedule): sched = [gain_expression[n] | gain_gesture[n] | phi_expression,
    // phi_gesture] (device fp32, context-owned, read by the mix kernels when they run), rescale[m] = the host's phi_m > 0 (the second launch is
    // issued).  Where the batch is doubled, encoder m mixes with s_eff = 1 + gain[m][t_b] (s_b - 1); sched == null: no schedule, the plain mix.
    // The single transformer reads row 0.
    virtual int set_guidance_schedule(const float* sched, int n_steps, bool rescale_expression, bool rescale_gesture) = 0;
    // one modality alone (DenoiserContext::set_modality): the Part this instance launches from now on, and its clips' rows of the track
    virtual int set_modality(int modality, const float* track) = 0;
    //   set_part(p): the Part the next evaluations run, for the pipelined loop (an encoder alone computes its head, EVAL_PLAIN, or restores its own
    //                share of it from the timestep cache, EVAL_RESTORE)
    //   import_expr(src, s): copy src's expression x0 estimate (what the gesture encoder reads) into this instance, on stream s
    virtual int set_part(int part) = 0;
    virtual int import_expr(const DenoiserInstance& src, hipStream_t s) = 0;
    // second instance sharing the finalized weights, working on another stream (null if not finalized)
    virtual DenoiserInstance* clone_shared(hipStream_t) = 0;
    // record `ev` on this instance's stream after the n-th token-per-lane launch of every eval (phase offset of a twin)
    virtual void notify_after_launches(hipEvent_t ev, int n) = 0;
    virtual double issued_flops_per_eval() const = 0;   // MFMA GEMM flops actually launched for the current (B,T)
    virtual size_t weight_bytes() const = 0;
    // debug taps (device -> caller device buffer, fp32): "aud_feat" [B,T,128], "expr_x0" [B,T,E]
    virtual int debug_copy(const std::string& what, float* out) = 0;
    int batch = 0, frames = 0;
    // Hint for the next evaluations: every row of `t` holds the SAME timestep (true in every sampling loop: gaussian_diffusion.py:
    // 1125, :792 build t = [i] * batch).  The time / speaker / FiLM embedding Linears (transformer.py:446-457, :77) then run on the
    // DISTINCT (timestep, speaker) rows only — the distinct speakers found at set_condition() — and are expanded per clip.
    // dsh_eval() checks the caller's tensor; the sampler sets it.
    bool t_uniform = false;
    Profiler* prof = nullptr;   // owned by the context; may be null
};

// What a dsh_ctx owns and the Sampler receives: the context-owned copies of the conditioning, the lengths and the expression track, and every
// instance that evaluates them — the whole-batch instance on the context stream (it owns the weights), the sub-batch instances, the
// side-stream prefetch instance and the gesture-side twin, each on a stream the context creates.  Implemented in denoiser_context.hip.
class DenoiserContext {
  public:
    virtual ~DenoiserContext() {}
    virtual int finalize(const std::map<std::string, HostTensor>& w) = 0;
    // The conditioning of DenoiserInstance::set_condition(), copied into context-owned memory in stream order.
    // Ragged batches: clip b of the padded batch [B, T, ...] has lengths[b] <= T valid frames.  Frames [0, lengths[b]) of every output are what
    // the clip gives evaluated alone at T = lengths[b], whatever the padded frames of any input hold; padded output frames are unspecified.
    // Only two operations of the model couple frames of a clip: the linear attention (time-softmax of K, k^T v) and the two k = 3 convolutions
    // of hubert_encoder — those read the lengths, everything else is per token and runs on the padded rows as it stands.  So regime decisions
    // (sub-batch split, kernel families, check_shape) and the flop count keep using B x T.
    //   lengths_host [B] int32 (host), null = all full; -1 before any state changes on a length < 1 or > T.
    //   lengths_host(): the current condition's lengths (null = all full), for the sampler's per-row noise streams and final zeroing.
    virtual int set_condition(int B, int T, const int32_t* lengths_host, const float* audio, const float* person_id, const float* hubert) = 0;
    virtual const int32_t* lengths_host() const = 0;
    virtual const int* lengths_dev() const = 0;
    virtual int batch() const = 0;
    virtual int frames() const = 0;
    virtual int gesture_channels() const = 0;            // channels [0, g) belong to the gesture encoder, [g, C) to the expression encoder; -1: one encoder
    // One modality alone (UniDiffuser only).  Part of the condition: set_condition() resets it to 0, set_modality() follows it.
    //   0 both: the joint evaluation.  1 expression: encoder_aud + encoder_exp run, no gesture-encoder launch is issued.  2 gesture:
    //   encoder_aud + encoder_ges run, and the gesture encoder reads `expression` [B, T, E] (device fp32, standardised, the clean track)
    //   wherever the joint evaluation reads the expression encoder's x0 estimate; the expression encoder is not launched.
    // The track is copied into context-owned memory in stream order and packed once (launch_pack_expr_track) into every evaluating
    // instance's expr_x0 / expr16 — a sub-batch instance takes its own clips' rows.  Every decision taken by token rows (sub-batch split,
    // kernel families, graph and timestep-cache range) stays that of the joint run of the same (B, T), so the active columns of a partial
    // evaluation are the joint evaluation's, bit for bit, given the same expression input.  Distinct from the pipelined loop's transient
    // set_part(): that loop is not entered while a modality is set.  -1 before any state changes on an unknown value, a single-transformer
    // model, no condition, or modality 2 without a track.
    //   modality_track(): the context-owned copy of the track while the modality is 2 (what the sampler writes into the expression columns
    //   of its result), else null.
    virtual int set_modality(int modality, const float* expression) = 0;
    virtual int modality() const = 0;
    virtual const float* modality_track() const = 0;
    virtual int set_guidance(const float* scale, int scale_row, bool doubled) = 0;   // as DenoiserInstance's, for every instance that evaluates
    virtual int set_guidance_schedule(const float* sched, int n_steps, bool rescale_expression, bool rescale_gesture) = 0;   // likewise (not per clip: no slices)
    // eps[B,T,C] = model(x[B,T,C], t[B]) with c1/c2 [B] (device fp32) feeding the expression x0; eval_level(): with the timestep cache (EvalMode)
    virtual int eval(const float* x, const int64_t* t, const float* c1, const float* c2, float* eps) = 0;
    virtual int eval_level(const float* x, const int64_t* t, const float* c1, const float* c2, float* eps, int mode, const int64_t* level) = 0;
    //   level_cache_prepare(n): as DenoiserInstance's, for the whole batch on one stream
    //   level_prefetch(t_values, n_levels, order, n_order, begin): enqueue that side-stream computation for the levels in `order`
    //   (t_values[level] = model timestep).  begin = 1 starts a run (conditions the side instance; -1 if prefetching is not
    //   available: then use modes 1 / 2 inline), begin = 0 appends further levels of the same run — the sampler enqueues each
    //   level one evaluation ahead of its first use, so the host never queues more than one level in front of the main chain.
    //   Every evaluation of such a run uses mode 2 and calls level_wait(level) before the first use of a level.
    virtual int level_cache_prepare(int n_levels) = 0;
    virtual int level_prefetch(const int64_t* t_values_host, int n_levels, const int* order, int n_order, int begin) = 0;
    virtual int level_wait(int level) = 0;
    // Sub-batch streams.  Large batches are conditioned as several independent sub-batches, each with its own instance (shared
    // weights) and stream.  eval() forks / joins them around ONE evaluation; a sampling loop can do better: clips never interact,
    // so it drives every sub-batch through ALL its steps on that sub-batch's stream and joins once at the end (sampler.hip).
    // sub_count() is valid after set_condition(); sub_get(i): the instance, its stream, and its clips [first, first + n).
    virtual int sub_count() const = 0;
    virtual int sub_get(int i, DenoiserInstance** inst, hipStream_t* stream, int* first_clip, int* n_clips) = 0;
    // Pipelined small-batch loop (round 6).  In the UniDiffuser the expression encoder sees only the expression channels of x, the gesture
    // encoder the gesture channels plus the expression encoder's x0 estimate of the SAME step (transformer.py:741-768), and every sampler update
    // is element-wise: the expression chain E_0 -> E_1 -> ... never waits for a gesture evaluation, only G_k waits for E_k.  A launch-bound
    // loop therefore runs the two encoders on two streams, G one step behind E: (n + 1) encoder times instead of 2 n.
    //   pipe_begin(&twin, &stream): the gesture-side twin of the whole-batch instance (shared weights, own workspace and stream,
    //                conditioned like it, reading its timestep-cache slots) and puts both into their part; -1 if not available
    //                (single transformer, split batch, no timestep cache, DSH_PIPE=0).  pipe_end(): both back to whole evaluations.
    //   import_expr_into_twin(s): the twin takes the whole-batch instance's expression x0 estimate, on stream s
    //   level_wait_stream(level, s): as level_wait(), for the twin's stream
    virtual int pipe_begin(DenoiserInstance** twin, hipStream_t* stream) = 0;
    virtual int pipe_end() = 0;
    virtual int import_expr_into_twin(hipStream_t s) = 0;
    virtual int level_wait_stream(int level, hipStream_t s) = 0;
    //   loop_begin(unsplit): called by the sampler before it asks for sub-batches, with the decision loop_regime() took (loop_regime.h); the
    //                context decides nothing here.  unsplit: the batch is conditioned as ONE batch for this loop (re-conditioned if it is split
    //                now) and marked so until loop_end(), and the next set_condition of the same shape skips the split too (sticky shape).
    //                Else the sticky shape is forgotten and the split stays.  Plain evaluations (dsh_eval) keep the sub-batch streams.
    //   unsplit_rows(): DSH_PIPE_ROWS as this context read it when it was created — the row limit of `unsplit`, handed to loop_regime() as a fact
    virtual int loop_begin(bool unsplit) = 0;
    virtual int loop_end() = 0;
    virtual size_t unsplit_rows() const = 0;
    virtual double issued_flops_per_eval() const = 0;   // MFMA GEMM flops actually launched for the current (B,T)
    virtual size_t weight_bytes() const = 0;
    virtual int debug_copy(const std::string& what, float* out) = 0;   // as DenoiserInstance's, every sub-batch instance its own clips' rows
    virtual void set_profiler(Profiler* p) = 0;         // owned by the dsh_ctx; may be null
    bool t_uniform = false;                             // the hint of DenoiserInstance::t_uniform, handed to every instance that evaluates
};

// DSH_EMB_DEDUP=0 (A/B switch): the embedding Linears run on every clip's row as before round 6
inline bool emb_dedup_enabled() { return switch_int(SW_EMB_DEDUP) != 0; }

DenoiserInstance* make_denoiser_instance(const ModelConfig& cfg, hipStream_t stream);   // the weight-owning instance (denoiser.hip); null: unknown precision
DenoiserContext* make_denoiser(const ModelConfig& cfg, hipStream_t stream);

}  // namespace dsh
