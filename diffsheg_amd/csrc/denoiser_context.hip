// DenoiserContext (denoiser.h): the context-owned conditioning and the per-stream instances that evaluate it; the model is Denoiser<T> (denoiser.hip)
#include <algorithm>

#include "denoiser.h"
#include "loop_regime.h"

namespace dsh {

namespace {

// Large batches are evaluated as two or three (DSH_DUAL=n: at most n) independent sub-batches on as many streams (the extra instances
// share the weights).  Clips never interact inside the denoiser, so this changes no result; the second stream starts a few
// launches late, which keeps the two kernel sequences out of phase: an HBM-bound StylizationBlock launch of one
// sub-batch then shares the chip with an MFMA-bound q|k|v / FFN launch of the other, and one launch's load prologue
// and tail run under the other's main loop (sty + ffn.linear2 pair: 566 -> 492 us, scripts/bench_tl_overlap.py).
class Context final : public DenoiserContext {
  public:
    Context(DenoiserInstance* primary, const ModelConfig& c, hipStream_t s) : cfg_(c), st_(s) {
        inst_.emplace_back(primary);
        nsplit_ = dual_streams();                            // off is "0"; n >= 2: at most n streams
        lag_ = (int)switch_int(SW_DUAL_LAG);
        // fp32 parity path: one GEMM launch of the config-2 batch (8704 rows) is only 1 - 3 rounds of co-resident tiles, so the
        // second stream's launches fill the partial last rounds (+1.5 % measured); bf16: from 12288 rows (want_split)
        // fp32 path: two streams from 4096 rows, three from 8700 (the 256-clip BEAT batch of configs[1]: 8704 rows = 17 x 512, every
        // Linear a 1.06 / 2.1 / 3.2-round launch of 64 x 64 tiles whose tail another sub-batch fills; measured 24.8 k -> 25.1 k frames/s)
        if (c.fp32_storage()) { min_rows_ = 4096; rows_per_stream_ = 2900; }
        if (const long rs = switch_positive(SW_DUAL_ROWS)) rows_per_stream_ = (size_t)rs;
        if (const long mr = switch_positive(SW_DUAL_MIN_ROWS)) min_rows_ = (size_t)mr;
        unsplit_rows_ = pipe_rows_context();
    }
    ~Context() override {
        (void)hipDeviceSynchronize();                        // side streams may still be running a level ahead of an aborted loop
        tw_.inst.reset();
        if (tw_.stream) (void)hipStreamDestroy(tw_.stream);
        if (tw_.ev) (void)hipEventDestroy(tw_.ev);
        pf_.prep.reset();                                    // the side instance borrows the whole-batch instance's slots and weights
        while (inst_.size() > 1) inst_.pop_back();
        for (hipStream_t st : streams_) (void)hipStreamDestroy(st);
        for (hipEvent_t ev : events_) (void)hipEventDestroy(ev);
        if (cond_buf_) (void)hipFree(cond_buf_);
        if (len_buf_) (void)hipFree(len_buf_);
        if (track_buf_) (void)hipFree(track_buf_);
        if (pf_.stream) (void)hipStreamDestroy(pf_.stream);
        for (hipEvent_t ev : pf_.lvl_ev) (void)hipEventDestroy(ev);
        if (pf_.ev_fork) (void)hipEventDestroy(pf_.ev_fork);
        if (pf_.ev_done) (void)hipEventDestroy(pf_.ev_done);
        if (pf_.t_dev) (void)hipFree(pf_.t_dev);
    }
    int finalize(const std::map<std::string, HostTensor>& w) override { return inst_[0]->finalize(w); }
    // (the whole-batch instance alone is profiled: a profiled batch is never split, the side instances never profiled)
    void set_profiler(Profiler* p) override { prof_ = p; inst_[0]->prof = p; }
    const int32_t* lengths_host() const override { return lens_ ? lens_host_.data() : nullptr; }
    const int* lengths_dev() const override { return lens_; }
    int batch() const override { return cond_.B; }
    int frames() const override { return cond_.T; }
    int modality() const override { return mod_; }
    int set_condition(int B, int T, const int32_t* lengths_host, const float* audio, const float* person_id, const float* hubert) override {
        DSH_REQUIRE(B > 0 && T > 0 && audio && person_id && hubert, "set_condition: null conditioning pointer / empty batch");
        if (lengths_host) {
            for (int b = 0; b < B; ++b)
                if (lengths_host[b] < 1 || lengths_host[b] > T) {
                    set_last_error("set_condition_ragged: clip " + std::to_string(b) + " has length " + std::to_string(lengths_host[b]) +
                                   ", valid lengths are 1 .. " + std::to_string(T) + " (the padded frame count)");
                    return -1;
                }
        }
        if (int e = inst_[0]->check_shape(B, T)) return e;          // (before any state changes: a refused shape leaves the previous condition usable)
        // The split (one stream vs sub-batches on several) may change between evals (profiler on/off), which re-runs the
        // per-instance set_condition: the conditioning is therefore copied into context-owned buffers, so the caller's
        // tensors only need to stay valid until this call's work on the context stream has been enqueued (stream order).
        const size_t na = (size_t)B * T * cfg_.audio_dim, np = (size_t)B * cfg_.style_dim, nh = (size_t)B * T * cfg_.hubert_dim;
        // the prefetch instance reads the previous conditioning on its own stream: order the overwrite behind it
        if (pf_.busy) { DSH_HIP_CHECK(hipStreamWaitEvent(st_, pf_.ev_done, 0)); pf_.busy = false; }
        if (tw_.busy) { DSH_HIP_CHECK(hipEventRecord(tw_.ev, tw_.stream)); DSH_HIP_CHECK(hipStreamWaitEvent(st_, tw_.ev, 0)); tw_.busy = false; }
        tw_.cond_ok = false;
        (void)inst_[0]->set_part(PART_BOTH);
        // the modality is part of the condition: a new condition is a joint one until set_modality() says otherwise
        mod_ = PART_BOTH;
        for (auto& in : inst_) (void)in->set_modality(PART_BOTH, nullptr);
        if (pf_.prep) (void)pf_.prep->set_modality(PART_BOTH, nullptr);
        if (tw_.inst) (void)tw_.inst->set_modality(PART_BOTH, nullptr);
        if (na + np + nh > cond_cap_) { if (int e = grow_device_buffer(cond_buf_, cond_cap_, na + np + nh, st_)) return e; }
        float* a = cond_buf_; float* p = a + na; float* h = p + np;
        DSH_HIP_CHECK(hipMemcpyAsync(a, audio, na * sizeof(float), hipMemcpyDeviceToDevice, st_));
        DSH_HIP_CHECK(hipMemcpyAsync(p, person_id, np * sizeof(float), hipMemcpyDeviceToDevice, st_));
        DSH_HIP_CHECK(hipMemcpyAsync(h, hubert, nh * sizeof(float), hipMemcpyDeviceToDevice, st_));
        // per-clip lengths: context-owned like the conditioning, read by the kernels when they run; instance i of a split sees `lens_ + its first clip`
        if (lengths_host) {
            if ((size_t)B > len_cap_) { if (int e = grow_device_buffer(len_buf_, len_cap_, (size_t)B, st_)) return e; }
            lens_host_.assign(lengths_host, lengths_host + B);
            // (pageable host source: staged before the call returns)
            DSH_HIP_CHECK(hipMemcpyAsync(len_buf_, lens_host_.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, st_));
            lens_ = len_buf_;
        } else lens_ = nullptr;
        cond_ = {B, T, a, p, h};
        return apply_condition(split_of_condition(B, T));
    }
    int set_modality(int m, const float* expression) override {
        DSH_REQUIRE(m >= 0 && m <= 2, "set_modality: unknown modality (0 both / 1 expression / 2 gesture)");
        DSH_REQUIRE(m == 0 || !cfg_.single_transformer, "set_modality: a single MotionTransformer has no separate expression / gesture encoders");
        DSH_REQUIRE(cond_.B > 0, "set_condition() must precede set_modality()");
        DSH_REQUIRE(m != 2 || expression, "set_modality: the gesture modality needs the expression track [B, T, expression_dim]");
        if (m == PART_GESTURE) {
            // context-owned copy, in stream order like the other conditioning tensors: a re-split re-packs from it (apply_condition), and the
            // sampler writes it into the expression columns of its result
            const size_t ne = (size_t)cond_.B * cond_.T * cfg_.expression_dim;
            // (the whole device: the sub-batch instances read the track on their own streams)
            if (ne > track_cap_) { if (int e = grow_device_buffer(track_buf_, track_cap_, ne, st_, true)) return e; }
            DSH_HIP_CHECK(hipMemcpyAsync(track_buf_, expression, ne * sizeof(float), hipMemcpyDeviceToDevice, st_));
        }
        mod_ = m;
        return push_modality(split_now_);
    }
    const float* modality_track() const override { return mod_ == PART_GESTURE ? track_buf_ : nullptr; }
    int eval(const float* x, const int64_t* t, const float* c1, const float* c2, float* eps) override {
        DSH_REQUIRE(cond_.B > 0, "set_condition() must precede eval()");
        const int ns = split_of_eval();
        if (ns != split_now_) { if (int e = apply_condition(ns)) return e; }   // e.g. the profiler was switched on in between
        for (auto& in : inst_) in->t_uniform = t_uniform;
        note_launch_value(LC_EVAL_STREAMS, ns);
        if (ns == 1) return inst_[0]->eval_level(x, t, c1, c2, eps, EVAL_PLAIN, nullptr);
        const int C = cfg_.channels();
        return fork_join(ns, [&](int i, hipStream_t si) -> int {
            const int b0 = first_clip(i, ns);
            const size_t off = (size_t)b0 * cond_.T * C;
            if (i > 0) DSH_HIP_CHECK(hipStreamWaitEvent(si, ev_lag_[i - 1], 0));      // a few launches behind sub-batch i - 1
            inst_[i]->notify_after_launches(i + 1 < ns ? ev_lag_[i] : nullptr, i + 1 < ns ? lag_ : 0);
            return inst_[i]->eval_level(x + off, t + b0, c1 + b0, c2 + b0, eps + off, EVAL_PLAIN, nullptr);
        });
    }
    int sub_count() const override { return (cond_.B > 0 && (split_now_ == 1 || want_split(cond_.B, cond_.T) == split_now_)) ? split_now_ : 1; }
    int sub_get(int i, DenoiserInstance** inst, hipStream_t* stream, int* first, int* n) override {
        DSH_REQUIRE(i >= 0 && i < split_now_ && split_now_ > 1 && inst && stream && first && n, "sub_get: no such sub-batch");
        *inst = inst_[i].get();
        *stream = i == 0 ? st_ : streams_[i - 1];
        *first = first_clip(i, split_now_);
        *n = first_clip(i + 1, split_now_) - *first;
        return 0;
    }
    int level_cache_prepare(int n_levels) override {
        if (cond_.B <= 0 || split_now_ != 1) return -1;
        return inst_[0]->level_cache_prepare(n_levels);
    }
    // Prefetch: a second instance (shared weights, own workspace) computes the x-independent head of every scheduled level on a
    // side stream, ahead of the loop, into the main instance's cache slots.  At launch-bound batch sizes the main chain keeps a
    // handful of CUs busy, so the side stream runs beside it: the 27 launches (0.28 ms at B = 1) leave every evaluation's
    // critical path, also for schedules that visit each level once (the first window of a chain).  DSH_LEVEL_PREFETCH=0: off.
    int level_prefetch(const int64_t* t_values_host, int n_levels, const int* order, int n_order, int begin) override {
        if (n_levels <= 0 || n_order < 0 || !t_values_host || (n_order > 0 && !order)) return -1;
        if (split_now_ != 1) return -1;                                     // the whole batch on one stream only
        const int nb = cond_.B;
        Prefetch& f = pf_;
        if (begin) {
            f.active = false;
            if (switch_int(SW_LEVEL_PREFETCH) == 0) return -1;
            if (level_cache_prepare(n_levels) != 0) return -1;
            char* slots = nullptr; size_t stride = 0; int nslots = 0;
            if (inst_[0]->level_slots(&slots, &stride, &nslots) != 0 || nslots < n_levels) return -1;
            if (!f.prep) {
                DSH_HIP_CHECK(hipStreamCreateWithFlags(&f.stream, hipStreamNonBlocking));
                DSH_HIP_CHECK(hipEventCreateWithFlags(&f.ev_fork, hipEventDisableTiming));
                DSH_HIP_CHECK(hipEventCreateWithFlags(&f.ev_done, hipEventDisableTiming));
                f.prep.reset(inst_[0]->clone_shared(f.stream));
                DSH_REQUIRE(f.prep != nullptr, "weights not finalized");
            }
            while ((int)f.lvl_ev.size() < n_levels) { hipEvent_t ev; DSH_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); f.lvl_ev.push_back(ev); }
            const size_t need = (size_t)n_levels * (nb + 1);
            if (need > f.t_cap) { if (int e = grow_device_buffer(f.t_dev, f.t_cap, need, f.stream)) return e; }
            // everything already enqueued on the evaluating stream (the conditioning copies, the previous run's last restore from
            // the slots) precedes the side stream's work
            DSH_HIP_CHECK(hipEventRecord(f.ev_fork, st_));
            DSH_HIP_CHECK(hipStreamWaitEvent(f.stream, f.ev_fork, 0));
            if (int e = f.prep->set_lengths(lens_)) return e;
            if (int e = f.prep->set_modality(mod_, nullptr)) return e;           // (fills the active encoder's share of every slot only)
            if (int e = f.prep->set_condition_light(nb, cond_.T, cond_.audio, cond_.pid)) return e;
            if (int e = f.prep->adopt_level_slots(slots, stride, nslots)) return e;
            f.levels = n_levels; f.nb = nb;
            f.active = true;
        }
        DSH_REQUIRE(f.active && n_levels == f.levels && nb == f.nb, "level_prefetch: no run in progress");
        int64_t* idx = f.t_dev + (size_t)n_levels * nb;                     // [n_levels] slot indices 0 .. n-1
        for (int i = 0; i < n_order; ++i) {
            const int k = order[i];
            DSH_REQUIRE(k >= 0 && k < n_levels, "level_prefetch: level out of range");
            int64_t* tk = f.t_dev + (size_t)k * nb;
            if (int e = launch_fill_i64(tk, t_values_host[k], (size_t)nb, f.stream)) return e;
            if (int e = launch_fill_i64(idx + k, (int64_t)k, 1, f.stream)) return e;
            f.prep->t_uniform = emb_dedup_enabled();                        // (tk was just filled with one value)
            if (int e = f.prep->eval_level(nullptr, tk, nullptr, nullptr, nullptr, EVAL_HEAD_ONLY, idx + k)) return e;
            DSH_HIP_CHECK(hipEventRecord(f.lvl_ev[k], f.stream));
        }
        DSH_HIP_CHECK(hipEventRecord(f.ev_done, f.stream));
        f.busy = true;
        return 0;
    }
    // ---- pipelined small-batch loop (denoiser.h): the gesture-side twin of the whole-batch instance -----------------------------
    int pipe_begin(DenoiserInstance** twin, hipStream_t* stream) override {
        if (switch_int(SW_PIPE) == 0 || cfg_.single_transformer || cond_.B <= 0 || split_now_ != 1 || !twin || !stream) return -1;
        if (mod_ != PART_BOTH) return -1;                                          // one modality alone: one chain, nothing to pipeline
        // (DDIM loops: the twin restores its head from the slots the prefetch run fills; loops without a timestep cache — DDPM — compute it)
        char* slots = nullptr; size_t stride = 0; int nslots = 0;
        const bool have_slots = pf_.active && inst_[0]->level_slots(&slots, &stride, &nslots) == 0;
        Twin& w = tw_;
        if (!w.inst) {
            // (default priority: a lowest-priority gesture stream was measured — single clip 16.6 -> 77 ms, profiles/r06b_ar_ab_twin_stream_priority.txt)
            DSH_HIP_CHECK(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
            DSH_HIP_CHECK(hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
            w.inst.reset(inst_[0]->clone_shared(w.stream));    // (never profiled: its prof stays null)
            DSH_REQUIRE(w.inst != nullptr, "weights not finalized");
            w.cond_ok = false;
        }
        // everything already enqueued on the evaluating stream (the conditioning copies) precedes the twin's work
        DSH_HIP_CHECK(hipEventRecord(w.ev, st_));
        DSH_HIP_CHECK(hipStreamWaitEvent(w.stream, w.ev, 0));
        if (int e = w.inst->set_guidance(gs_, gs_row_, gs_dbl_)) return e;
        if (int e = w.inst->set_guidance_schedule(sched_, sched_n_, sched_rs_[0], sched_rs_[1])) return e;
        if (!w.cond_ok) {
            if (int e = w.inst->set_part(PART_BOTH)) return e;
            if (int e = w.inst->set_lengths(lens_)) return e;
            if (int e = w.inst->set_condition(cond_.B, cond_.T, cond_.audio, cond_.pid, cond_.hubert)) return e;
            w.cond_ok = true;
        }
        if (have_slots) { if (int e = w.inst->adopt_level_slots(slots, stride, nslots)) return e; }
        if (int e = w.inst->set_part(PART_GESTURE)) return e;
        if (int e = inst_[0]->set_part(PART_EXPRESSION)) return e;
        w.inst->t_uniform = t_uniform; inst_[0]->t_uniform = t_uniform;
        w.busy = true;
        *twin = w.inst.get(); *stream = w.stream;
        return 0;
    }
    int pipe_end() override {
        if (tw_.inst) (void)tw_.inst->set_part(PART_BOTH);
        return inst_[0]->set_part(PART_BOTH);
    }
    int import_expr_into_twin(hipStream_t s) override {
        DSH_REQUIRE(tw_.inst, "import_expr: no pipelined run in progress");
        return tw_.inst->import_expr(*inst_[0], s);
    }
    int loop_begin(bool unsplit) override {
        if (cond_.B <= 0) return 0;
        if (!unsplit) { loop_.sticky_B = loop_.sticky_T = 0; return 0; }
        loop_.sticky_B = cond_.B; loop_.sticky_T = cond_.T; loop_.unsplit = true;
        if (split_now_ != 1) return apply_condition(1);
        return 0;
    }
    int loop_end() override { loop_.unsplit = false; return 0; }
    size_t unsplit_rows() const override { return unsplit_rows_; }
    int gesture_channels() const override { return cfg_.single_transformer ? -1 : cfg_.dim_pose; }
    int level_wait_stream(int level, hipStream_t s) override {
        DSH_REQUIRE(level >= 0 && level < (int)pf_.lvl_ev.size(), "level_wait_stream: level out of range");
        DSH_HIP_CHECK(hipStreamWaitEvent(s, pf_.lvl_ev[level], 0));
        return 0;
    }
    int level_wait(int level) override { return level_wait_stream(level, st_); }
    int eval_level(const float* x, const int64_t* t, const float* c1, const float* c2, float* eps, int mode, const int64_t* level) override {
        if (mode == EVAL_PLAIN) return eval(x, t, c1, c2, eps);
        DSH_REQUIRE(cond_.B > 0 && split_now_ == 1, "eval_level: the timestep cache is a single-stream feature");
        inst_[0]->t_uniform = t_uniform;
        return inst_[0]->eval_level(x, t, c1, c2, eps, mode, level);
    }
    double issued_flops_per_eval() const override {
        double f = 0;
        for (int i = 0; i < split_now_; ++i) f += inst_[i]->issued_flops_per_eval();
        return f;
    }
    size_t weight_bytes() const override { return inst_[0]->weight_bytes(); }
    // every instance that evaluates sees the context's scales: a sub-batch instance its clips' slice (per-clip scales), the gesture twin all
    int set_guidance(const float* scale, int scale_row, bool doubled) override {
        gs_ = scale; gs_row_ = scale_row ? 1 : 0; gs_dbl_ = doubled;
        for (int i = 0; i < (int)inst_.size(); ++i) { if (int e = push_guidance(i, split_now_)) return e; }
        if (tw_.inst) { if (int e = tw_.inst->set_guidance(gs_, gs_row_, gs_dbl_)) return e; }
        return 0;
    }
    // ... and the context's schedule: one table for every clip, so every instance takes the same pointer (the prefetch instance never mixes)
    int set_guidance_schedule(const float* sched, int n_steps, bool rescale_expression, bool rescale_gesture) override {
        sched_ = sched; sched_n_ = sched ? n_steps : 0; sched_rs_[0] = sched && rescale_expression; sched_rs_[1] = sched && rescale_gesture;
        for (auto& in : inst_) { if (int e = in->set_guidance_schedule(sched_, sched_n_, sched_rs_[0], sched_rs_[1])) return e; }
        if (tw_.inst) { if (int e = tw_.inst->set_guidance_schedule(sched_, sched_n_, sched_rs_[0], sched_rs_[1])) return e; }
        return 0;
    }
    int debug_copy(const std::string& what, float* out) override {
        if (split_now_ == 1) return inst_[0]->debug_copy(what, out);
        // sub-batch streams: every instance copies its own clips' rows on its own stream, joined into the context stream
        const int w = what == "aud_feat" ? cfg_.audio_dim : cfg_.expression_dim;
        return fork_join(split_now_, [&](int i, hipStream_t) -> int {
            return inst_[i]->debug_copy(what, out + (size_t)first_clip(i, split_now_) * cond_.T * w);
        });
    }

  private:
    struct Cond { int B = 0, T = 0; const float* audio = nullptr; const float* pid = nullptr; const float* hubert = nullptr; };
    int want_split(int B, int T) const {
        if (nsplit_ < 2 || (prof_ && prof_->on) || (size_t)B * T < min_rows_) return 1;
        // Two streams from min_rows_ token rows, three from 3 * rows_per_stream_ = 64 500 (the 950-clip batch of configs[2]: 83 600).
        // Measured on MI355X with the sampling loop's free-running sub-batch streams (sampler.hip; round 3), frames/s at
        // 1 / 2 / 3 streams: 100 clips (8.8k rows) 83.0k / 81.6k / -; 200 clips 87.6k / 112.4k / 107.4k; 475 clips 111.6k / 129.6k /
        // 125.8k; 650 clips - / 134.8k / 133.2k; 800 clips - / 129.9k / 134.9k; 950 clips - / 133.0k / 136.2k (four: 121k; a disjoint
        // CU partition per stream through hipExtStreamCreateWithCUMask:
        // 100 - 118k).  With one fork / join per EVALUATION (dsh_eval) the same three streams give 130k at 950 clips.
        const int by_rows = std::max(2, (int)((size_t)B * T / rows_per_stream_));
        return std::min(std::min(nsplit_, by_rows), B);
    }
    // sub-batch i covers clips [first_clip(i), first_clip(i + 1)): equal shares, or (bench experiment) the cumulative boundaries of
    // DSH_SPLIT_AT="c1,c2,..." when they fit the batch and the stream count
    int first_clip(int i, int ns) const {
        static const std::vector<int> at = [] {
            std::vector<int> v;
            if (const char* e = switch_str(SW_SPLIT_AT)) { for (const char* p = e; *p;) { v.push_back(atoi(p)); while (*p && *p != ',') ++p; if (*p == ',') ++p; } }
            return v;
        }();
        if ((int)at.size() == ns - 1 && i > 0 && i < ns) {
            bool ok = at[0] > 0 && at.back() < cond_.B;
            for (size_t k = 1; k < at.size(); ++k) ok = ok && at[k] > at[k - 1];
            if (ok) return at[i - 1];
        }
        return (int)((int64_t)cond_.B * i / ns);
    }
    // One fork / join of the sub-batch streams around f(i, stream of instance i) for i in [0, ns): instance 0 works on the context stream, every
    // other on its own behind all the context stream holds so far, and the context stream goes on behind each of them.
    template <typename F> int fork_join(int ns, F&& f) {
        DSH_HIP_CHECK(hipEventRecord(ev_fork_, st_));
        for (int i = 0; i < ns; ++i) {
            hipStream_t si = i == 0 ? st_ : streams_[i - 1];
            if (i > 0) DSH_HIP_CHECK(hipStreamWaitEvent(si, ev_fork_, 0));
            if (int e = f(i, si)) return e;
            if (i > 0) {
                DSH_HIP_CHECK(hipEventRecord(ev_join_[i - 1], si));
                DSH_HIP_CHECK(hipStreamWaitEvent(st_, ev_join_[i - 1], 0));
            }
        }
        return 0;
    }
    int apply_condition(int ns) {
        while ((int)inst_.size() < ns) {
            hipStream_t st; hipEvent_t lag, join;
            DSH_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            streams_.push_back(st);
            DSH_HIP_CHECK(hipEventCreateWithFlags(&lag, hipEventDisableTiming)); events_.push_back(lag); ev_lag_.push_back(lag);
            DSH_HIP_CHECK(hipEventCreateWithFlags(&join, hipEventDisableTiming)); events_.push_back(join); ev_join_.push_back(join);
            if (!ev_fork_) { DSH_HIP_CHECK(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming)); events_.push_back(ev_fork_); }
            DenoiserInstance* c = inst_[0]->clone_shared(st);
            DSH_REQUIRE(c != nullptr, "weights not finalized");
            inst_.emplace_back(c);
        }
        split_now_ = ns;
        for (int i = 0; i < ns; ++i) { if (int e = push_guidance(i, ns)) return e; }
        for (int i = 0; i < ns; ++i) { if (int e = inst_[i]->set_guidance_schedule(sched_, sched_n_, sched_rs_[0], sched_rs_[1])) return e; }
        if (ns == 1) {
            if (int e = inst_[0]->set_lengths(lens_)) return e;
            if (int e = inst_[0]->set_condition(cond_.B, cond_.T, cond_.audio, cond_.pid, cond_.hubert)) return e;
            return mod_ ? push_modality(1) : 0;
        }
        if (int e = fork_join(ns, [&](int i, hipStream_t) -> int {
                const int b0 = first_clip(i, ns), nb = first_clip(i + 1, ns) - b0;
                const size_t ft = (size_t)b0 * cond_.T;
                if (int e = inst_[i]->set_lengths(lens_ ? lens_ + b0 : nullptr)) return e;
                return inst_[i]->set_condition(nb, cond_.T, cond_.audio + ft * cfg_.audio_dim, cond_.pid + (size_t)b0 * cfg_.style_dim,
                                               cond_.hubert + ft * cfg_.hubert_dim);
            })) return e;
        return mod_ ? push_modality(ns) : 0;
    }
    // the condition's modality to the ns evaluating instances (each packs its own clips' rows of the given track on its own stream, forked
    // from and joined into the context stream), to the prefetch instance and (unused: the pipelined loop is not entered) the twin
    int push_modality(int ns) {
        const size_t row = (size_t)cond_.T * cfg_.expression_dim;
        const float* tr = mod_ == PART_GESTURE ? track_buf_ : nullptr;
        auto pack = [&](int i, hipStream_t) -> int { return inst_[i]->set_modality(mod_, tr + (size_t)(ns > 1 ? first_clip(i, ns) : 0) * row); };
        if (tr) { if (int e = ns > 1 ? fork_join(ns, pack) : pack(0, st_)) return e; }
        for (int i = tr ? ns : 0; i < (int)inst_.size(); ++i) { if (int e = inst_[i]->set_modality(mod_, nullptr)) return e; }
        if (pf_.prep) { if (int e = pf_.prep->set_modality(mod_, nullptr)) return e; }
        if (tw_.inst) { if (int e = tw_.inst->set_modality(mod_, nullptr)) return e; }
        return 0;
    }
    // instance i of an ns-way split: the scales of its clips (first_clip(i, ns) onwards) when they are per clip
    int push_guidance(int i, int ns) {
        const int b0 = (gs_row_ && ns > 1 && i < ns && cond_.B > 0) ? first_clip(i, ns) : 0;
        return inst_[i]->set_guidance(gs_ ? gs_ + b0 : nullptr, gs_row_, gs_dbl_);
    }
    std::vector<std::unique_ptr<DenoiserInstance>> inst_;     // [0] owns the weights; the others share them
    const float* gs_ = nullptr; int gs_row_ = 0; bool gs_dbl_ = false;   // the context's guidance (set_guidance)
    const float* sched_ = nullptr; int sched_n_ = 0; bool sched_rs_[2] = {false, false};   // the context's guidance schedule (set_guidance_schedule)
    ModelConfig cfg_;
    Profiler* prof_ = nullptr;                             // owned by the dsh_ctx; may be null
    hipStream_t st_;
    std::vector<hipStream_t> streams_;
    std::vector<hipEvent_t> events_, ev_lag_, ev_join_;
    hipEvent_t ev_fork_ = nullptr;
    Cond cond_;
    float* cond_buf_ = nullptr;                            // context-owned copy of [audio | person_id | hubert]
    int* len_buf_ = nullptr; size_t len_cap_ = 0;          // ... and of the per-clip lengths of a ragged condition
    const int* lens_ = nullptr;                            // len_buf_ while the current condition is ragged, else null
    std::vector<int32_t> lens_host_;
    size_t cond_cap_ = 0;
    int mod_ = PART_BOTH;                                  // the condition's modality (set_modality)
    float* track_buf_ = nullptr; size_t track_cap_ = 0;    // context-owned copy of the given expression track [B, T, E] (modality 2)
    // side-stream producer of the x-independent head of the whole batch (level_prefetch)
    struct Prefetch {
        std::unique_ptr<DenoiserInstance> prep;             // shared weights, own workspace, conditioned with mel features + speaker only
        hipStream_t stream = nullptr;
        std::vector<hipEvent_t> lvl_ev;
        hipEvent_t ev_fork = nullptr, ev_done = nullptr;
        int64_t* t_dev = nullptr; size_t t_cap = 0;
        bool busy = false, active = false;
        int levels = 0, nb = 0;
    } pf_;
    // gesture-side twin of inst_[0] for the pipelined small-batch loop (pipe_begin)
    struct Twin {
        std::unique_ptr<DenoiserInstance> inst;            // shared weights, own workspace
        hipStream_t stream = nullptr; hipEvent_t ev = nullptr;
        bool cond_ok = false, busy = false;                // conditioned like inst_[0] for the current condition; may still be reading it on its stream
    } tw_;
    size_t unsplit_rows_ = 0;                              // DSH_PIPE_ROWS as read when this context was created: a fact of loop_regime(), not used here
    // what loop_begin() / loop_end() leave behind, and the one reader of each: the split of a new condition, the split of the next evaluation
    struct LoopState {
        int sticky_B = 0, sticky_T = 0;                    // shape whose last loop ran unsplit: set_condition conditions it as one batch
        bool unsplit = false;                              // a sampling loop is running this batch unsplit on purpose (its evaluations must not re-split it)
    } loop_;
    // (the one piece of the loop policy evaluated here, for the sticky shape: at set_condition time no run exists to decide it)
    int split_of_condition(int B, int T) const {
        const bool sticky = B == loop_.sticky_B && T == loop_.sticky_T;
        return (sticky && pipe_available(switch_int(SW_PIPE), switch_int(SW_LEVEL_PREFETCH), switch_int(SW_LEVEL_CACHE), gesture_channels(), prof_ && prof_->on))
                   ? 1 : want_split(B, T);
    }
    int split_of_eval() const { return (loop_.unsplit && split_now_ == 1) ? 1 : want_split(cond_.B, cond_.T); }
    int nsplit_ = 1, split_now_ = 1, lag_ = 0;             // (nsplit_, lag_, unsplit_rows_: from the switches, in the constructor)
    size_t min_rows_ = 12288;                              // batches below this many token rows run on one stream
    size_t rows_per_stream_ = 21500;                       // streams = rows / this (at least two, at most DSH_DUAL): three from 64 500 rows
};

}  // namespace

DenoiserContext* make_denoiser(const ModelConfig& cfg, hipStream_t stream) {
    DenoiserInstance* d = make_denoiser_instance(cfg, stream);
    return d ? new Context(d, cfg, stream) : nullptr;
}

}  // namespace dsh
