// Validation metrics on the device: the FGD pose encoder (pose_encoder.hip) and the per-batch metrics (metrics.hip).
// Reference: models/motion_autoencoder.py:38-100,192-204 (HalfEmbeddingNet / PoseEncoderConv in eval mode),
// trainers/ddpm_show_trainer.py:516-550, ddpm_beat_trainer.py:587-597 (MSE / PCK / diversity).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "denoiser.h"
#include "dsh_common.h"

namespace dsh {

// One Conv1d stage as an implicit NT GEMM on channels-last activations (no im2col buffer):
//   Y[b, t, n] = act(bias[n] + sum_{k < Kreal} X[b * x_clip + t * x_step + k] * W[n, k]),   row m = b * Tout + t.
// The im2col row of output frame t is the contiguous slice x[b, s t : s t + ksize, :] of a channels-last clip, so x_step = s * Cin and
// Kreal = ksize * Cin.  W is [N, Kp] with Kp = Kreal rounded up to the 32-float K tile, zero padded; the A-side loads of the pad are MASKED
// (never issued, zeros staged instead): nothing outside the Kreal floats of a row is ever read, whatever lies behind them.
struct ConvGemmArgs {
    const float* X; long long x_clip; int x_step;   // floats; all multiples of 4 (16-byte loads), X 16-byte aligned
    const float* W; int ldw;                        // [N, Kp]
    const float* bias;                              // [N]
    float* Y; long long y_clip;                     // Y[b * y_clip + t * N + n]; N % 4 == 0, y_clip % 4 == 0
    int Tout, M, N, Kreal, Kp;
    int leaky;                                      // 1: LeakyReLU(0.2) on (acc + bias)
    int nt_n, nt_m;                                 // (launcher)
};
int launch_conv_gemm_f32(const ConvGemmArgs& a, hipStream_t s);
// x[B, frames, C] -> y[B, n_poses, Cp] (first n_poses frames, channels zero padded to Cp): only for inputs the 16-byte operand loads
// cannot address in place (C % 4 != 0 or a misaligned pointer)
int launch_stage_clips(const float* x, int B, int frames, int C, float* y, int n_poses, int Cp, hipStream_t s);

class FgdEncoder {
public:
    FgdEncoder(int n_poses, int dim, int base, hipStream_t s);
    ~FgdEncoder();
    int load(const char* name, const float* host, const int64_t* shape, int ndim);
    int finalize();
    int encode(const float* x, int batch, int frames, float* latents);
    bool finalized() const { return finalized_; }
    int num_layers() const { return 4 + (int)lin_idx_.size() + 1; }
    // host only (no device needed): layer idx as finalize() would upload it; dims3 = {N, Kreal, Kp}, W [N, Kp], bias [N] (all nullable)
    int packed_layer(int idx, int32_t* dims3, float* W, float* bias) const;
private:
    struct Lin { float* W = nullptr; float* b = nullptr; int N = 0, Kreal = 0, Kp = 0; };
    int check_complete() const;
    int pack_layer(int idx, Lin* meta, std::vector<float>* wf, std::vector<float>* bf) const;
    int reserve(int batch);
    void release_buffers();
    int n_poses_, dim_, base_, Cp_;
    int T_[5];                               // frames after each conv stage (T_[0] = n_poses)
    hipStream_t stream_;                     // null until finalize(): a stream of its own is created there
    bool owns_stream_ = false;
    std::map<std::string, HostTensor> staged_;
    std::vector<std::pair<std::string, std::vector<int64_t>>> expected_;   // key -> shape, in the reference's registration order
    std::vector<int> lin_idx_, bn_idx_;      // out_net indices of the Linears and of the BatchNorm behind each (-1: none)
    bool finalized_ = false;
    Lin conv_[4];
    std::vector<Lin> lin_;                   // out_net Linears (BatchNorm folded) + fc_mu
    int cap_ = 0;
    float* xs_ = nullptr;                    // staged input (only when the caller's tensor cannot be addressed in place)
    float* act_[4] = {nullptr, nullptr, nullptr, nullptr};   // conv outputs; act_[3] = the flattened rows [B, Kp of the first Linear]
    std::vector<float*> lbuf_;               // outputs of the Linears but the last, [B, Kp of the next]
};

// ---- per-batch metrics (metrics.hip) --------------------------------------------------------------------------------
// result_dev (device, 8-byte aligned, DSH_METRICS_RESULT_BYTES(groups)): see include/diffsheg_hip.h
long long batch_metrics_result_bytes(int B, int T, int C, int b_div);
int launch_batch_metrics(const float* outputs, const float* motions, int B, int T, int C, int joint_dim, int b_div, void* result_dev,
                         hipStream_t s);

}  // namespace dsh
