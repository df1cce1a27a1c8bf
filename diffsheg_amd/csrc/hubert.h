// HuBERT encoder (the hubert-large family: "layer" feature-extractor norm with conv bias, stable-LayerNorm transformer), fp32 on the
// exact-fp32 matrix pipe: the second feature test_custom_aud (trainers/ddpm_show_trainer.py:944-1100) computes from a speech signal.
// Weights come by the state-dict keys of transformers' HubertModel; the architecture is that of its modeling_hubert.py.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "denoiser.h"
#include "dsh_common.h"

namespace dsh {

struct HubertConfig {
    int hidden, layers, heads, intermediate;
    int conv_dim[7], conv_kernel[7], conv_stride[7];
    int pos_kernel, pos_groups;
    float ln_eps;
};

// h_out[b, t, o] = h[b, t, o] + GELU(bias[o] + sum_{tap, i} W[o, tap cg + i] h[b, t + tap - pk / 2, g cg + i]),  g = o / cg: the grouped
// positional convolution (padding pk / 2, last output frame dropped, pk even) as one implicit GEMM per group; frames outside [0, M) are
// staged as zeros and never loaded.  h_out must not alias h.  lens (DEVICE int32 [B], nullable): row b owns lens[b] of its M frames (clamped to
// [0, M]); the frames behind count as zeros too and are never loaded, h_out is 0 there: row b has the bits of the dense call on it alone at
// M = lens[b].
int launch_pos_conv(const float* h, int B, int M, int hidden, int groups, int pk, const float* W, const float* bias, float* h_out, hipStream_t s,
                    const int* lens = nullptr);
// y[row] = act(LayerNorm(x[row]) gamma + beta) over C <= 1024 channels (two-pass moments), in place allowed; gelu = 1: erf-GELU behind it
// lens (DEVICE int32, nullable) with M: the rows are [rows / M, M] frames and frame t >= lens[b] is written as 0 without being read
int launch_ln_act_rows(const float* x, long long rows, int C, const float* gamma, const float* beta, float eps, int gelu, float* y, hipStream_t s,
                       const int* lens = nullptr, int M = 1);
// first feature-extractor layer: Conv1d(1, C, k, stride s, bias) -> LayerNorm(C) -> GELU, x [B, n] -> y [B, L, C] channels-last
int launch_conv0_ln_gelu(const float* x, int B, long long n, int L, int C, int k, int s, const float* W, const float* bias, const float* gamma,
                         const float* beta, float* y, hipStream_t st);

class HubertEncoder {
public:
    enum Kind { CONV = 0, FEAT_PROJ = 1, POS_CONV = 2, QKV = 3, OUT_PROJ = 4, FFN_IN = 5, FFN_OUT = 6 };
    static int validate(const HubertConfig& c);
    HubertEncoder(const HubertConfig& c, hipStream_t s);
    ~HubertEncoder();
    int load(const char* name, const float* host, const int64_t* shape, int ndim);
    int finalize();
    long long num_frames(long long n) const;      // -1 when n is shorter than the receptive field
    int receptive_field() const;
    void set_chunk_pass(int p) { pass_ = p < 1 ? 1 : p; }
    // Precision of the transformer layers (step 5 of run()), before finalize() only: FP32 (default) or BF16.  BF16: the four Linears of a layer
    // on the bf16 matrix pipe (gemm_bf16_pro.hip) with W' = RNE_bf16(gamma (.) W) rounded once from the fp64 fold, LayerNorm as normalise-then-
    // round in the staging registers, bf16 q|k|v, attention output and FFN hidden, softmax_attention_bf16_kernel; the residual stream h stays
    // fp32.  Everything in front of the layers and the last LayerNorm are the fp32 launches either way.  The layers' fp32 weights are not uploaded.
    enum Precision { FP32 = 0, BF16 = 1 };
    int set_precision(int p);
    int precision() const { return precision_; }
    // test tap: run() copies h [B M, hidden] as the positional convolution leaves it to this DEVICE buffer (null: off)
    void set_debug_tap(float* dev) { tap_ = dev; }
    int encode(const float* x, int B, long long n, float* out);
    // x [B, n_max] of which row b owns lens_samples[b] samples (HOST array): out [B, num_frames(n_max), hidden], row b bit for bit encode() of
    // its own samples alone, 0 behind its num_frames(lens_samples[b]) frames, whatever the samples behind hold.  -1 (nothing launched) for a
    // row shorter than the receptive field or longer than n_max.  Uploads the B frame counts once, which waits for the stream.
    int encode_ragged(const float* x, int B, long long n_max, const int64_t* lens_samples, float* out);
    // host only: one Linear / convolution as finalize() uploads it.  dims2 = {N, K}; W [N, K], bias [N], fc [N] (row sums of the folded
    // weight; zeros for the kinds without a folded LayerNorm); all nullable.  BF16 precision, the four layer kinds: W holds the bf16-rounded
    // weights as fp32 values and fc is zeros (that path has no fc vector).
    int debug_packed(int kind, int layer, int32_t* dims2, float* W, float* bias, float* fc) const;
private:
    struct Lin { float *W = nullptr, *b = nullptr, *c = nullptr; bf16* W16 = nullptr; int N = 0, K = 0; };
    struct Vec { float* g = nullptr; float* b = nullptr; };
    int check_complete() const;
    int pack(int kind, int layer, int* N, int* K, std::vector<float>* W, std::vector<float>* b, std::vector<float>* c,
             std::vector<uint16_t>* W16 = nullptr) const;
    bool layer_kind_bf16(int kind) const { return precision_ == BF16 && kind >= QKV && kind <= FFN_OUT; }
    int upload(int kind, int layer, Lin* out);
    int upload_ln(const std::string& key, int n, Vec* out);
    int reserve(int B, long long n);
    int run(const char* what, const float* x, int B, long long n, const int64_t* lens_samples, float* out);
    void release_buffers();
    const std::vector<float>& T(const std::string& k) const { return staged_.at(k).data; }
    HubertConfig cfg_;
    hipStream_t stream_;
    bool owns_stream_ = false, finalized_ = false;
    int pass_ = 4;                                // batch rows of the convolution stack per pass (its activations are 131 MB per 20 s row)
    std::map<std::string, HostTensor> staged_;
    std::vector<std::pair<std::string, std::vector<int64_t>>> expected_;
    Lin conv_[7], feat_proj_, pos_conv_;
    Vec conv_ln_[7], final_ln_;
    struct Layer { Lin qkv, out, ffn_in, ffn_out; };
    std::vector<Layer> layer_;
    std::vector<void*> owned_;                    // every weight allocation
    float *act_a_ = nullptr, *act_b_ = nullptr, *feat_ = nullptr, *h_ = nullptr, *h2_ = nullptr, *qkv_ = nullptr, *att_ = nullptr, *ffn_ = nullptr;
    bf16 *qkv16_ = nullptr, *att16_ = nullptr, *ffn16_ = nullptr;      // BF16 precision: the layers' activations (qkv_, att_, ffn_ stay null)
    float* mom_ = nullptr;                        // BF16 precision: (mean, rstd) per row in front of q|k|v and intermediate_dense
    float* tap_ = nullptr;
    int precision_ = FP32;
    long long cap_act_ = 0, cap_rows_ = 0;
    std::vector<int32_t> lens_host_;              // frame counts of the rows of an encode_ragged call, and their device copy
    int32_t* lens_dev_ = nullptr;
    int cap_lens_ = 0;
};

}  // namespace dsh
