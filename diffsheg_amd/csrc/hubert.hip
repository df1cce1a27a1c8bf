// HuBERT encoder, fp32 on the exact-fp32 matrix pipe (v_mfma_f32_32x32x2_f32).  The computation (transformers' modeling_hubert.py,
// feat_extract_norm = "layer", do_stable_layer_norm = True), on channels-last activations:
//   1. x [B, n], already normalised by the caller
//   2. seven times Conv1d (valid, stride s, bias) -> LayerNorm over the channels of a frame (eps 1e-5) -> erf-GELU
//        layer 0 (one input channel): conv0_ln_gelu_kernel, one wave per output frame, LayerNorm + GELU fused
//        layers 1 .. 6: the implicit GEMM of pose_encoder.hip (A row base t s C, K = k C contiguous) + ln_act_rows_kernel in place
//        The stack runs over at most `pass` batch rows at a time (131 MB of activations per 20 s row behind layer 0 at the large widths); every
//        output element has one accumulator with K ascending whatever the tile shape, so the pass size never changes a bit of the result.
//   3. LayerNorm(conv_dim) folded into the projection to `hidden` (pro 1 of gemm_f32_pro.hip)
//   4. h += GELU(posconv(h)): pos_conv_gemm_f32_kernel, an implicit GEMM per group (M = frames, N = channels of the group, K = taps x channels of
//      the group walked tap by tap at row stride `hidden`), frames outside [0, M) staged as zeros, GELU + residual in the epilogue
//   5. per layer: h += out_proj(softmax(q k^T) v) with q|k|v one pro-1 launch (first LayerNorm folded, q rows pre-scaled by 1 / 8),
//      softmax_attention_f32_kernel (audio_front.hip), out_proj a pro-0 launch with the residual;
//      h += output_dense(GELU(intermediate_dense(final_LN(h)))): pro 1 with the GELU epilogue, pro 0 with the residual
//      precision BF16 (set_precision, opt-in): the same step on the bf16 matrix pipe (gemm_bf16_pro.hip): row_moments_kernel + a Linear that
//      stages RNE_bf16((h - mean) rstd) in front of q|k|v and intermediate_dense, bf16 q|k|v / attention output / FFN hidden,
//      softmax_attention_bf16_kernel, both residual additions into the fp32 h in place; steps 1 - 4 and 6 are the fp32 launches either way
//   6. encoder.layer_norm
// Every reduction has a fixed order and there are no atomics: batch row b gives the same bits whatever B is.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "audio_front.h"
#include "dsh_kernels.h"
#include "fgd.h"
#include "hubert.h"

namespace dsh {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int HB_ROWS_PER_BLOCK = 4;     // one wave per row
constexpr int HB_PER_LANE = 16;          // rows of up to 1024 channels
constexpr float HB_CONV_LN_EPS = 1e-5f;  // nn.LayerNorm's default: the feature-extractor norms do not take config.layer_norm_eps

__device__ __forceinline__ float hb_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// two-pass LayerNorm of the row a wave holds in v[] (channel lane + 64 i), optional GELU, store
__device__ __forceinline__ void hb_ln_store(const float (&v)[HB_PER_LANE], int lane, int C, const float* __restrict__ gamma,
                                            const float* __restrict__ beta, float eps, int gelu, float* yrow) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < HB_PER_LANE; ++i) s += v[i];
    const float mean = hb_wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < HB_PER_LANE; ++i) {
        const float d = (lane + 64 * i < C) ? v[i] - mean : 0.f;
        q += d * d;
    }
    const float rstd = 1.0f / sqrtf(hb_wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < HB_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        if (c < C) {
            const float y = (v[i] - mean) * rstd * gamma[c] + beta[c];
            yrow[c] = gelu ? gelu_f(y) : y;
        }
    }
}

// (x and y may be the same rows: a wave has read its whole row before it stores any of it)
// lens (nullable): the rows are [B, M] frames and frame t >= lens[b] is written as 0 without being read.
__global__ __launch_bounds__(256) void ln_act_rows_kernel(const float* x, long long rows, int C, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, int gelu, float* y,
                                                          const int* __restrict__ lens, int M) {
    const long long row = (long long)blockIdx.x * HB_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    if (lens && row % M >= lens[row / M]) {
        for (int c = lane; c < C; c += 64) y[row * C + c] = 0.f;
        return;
    }
    const float* xr = x + row * C;
    float v[HB_PER_LANE];
#pragma unroll
    for (int i = 0; i < HB_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < C ? xr[c] : 0.f;
    }
    hb_ln_store(v, lane, C, gamma, beta, eps, gelu, y + row * C);
}

int launch_ln_act_rows(const float* x, long long rows, int C, const float* gamma, const float* beta, float eps, int gelu, float* y, hipStream_t s,
                       const int* lens, int M) {
    DSH_REQUIRE(x && y && gamma && beta && rows > 0 && C > 0 && C <= 64 * HB_PER_LANE, "ln_act_rows: rows of 1 .. 1024 channels");
    DSH_REQUIRE((rows + HB_ROWS_PER_BLOCK - 1) / HB_ROWS_PER_BLOCK < (1ll << 31), "ln_act_rows: too many rows");
    DSH_REQUIRE(!lens || (M >= 1 && rows % M == 0), "ln_act_rows: ragged rows are [B, M] frames");
    hipLaunchKernelGGL(ln_act_rows_kernel, dim3((unsigned)((rows + HB_ROWS_PER_BLOCK - 1) / HB_ROWS_PER_BLOCK)), dim3(256), 0, s, x, rows, C, gamma,
                       beta, eps, gelu, y, lens, M);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// One wave per output frame: the k samples of the frame are the same for every lane (broadcast loads), lane l owns channels l + 64 i.
// W [C, k] as the state dict has it ([C, 1, k]); taps ascending, then the bias.
__global__ __launch_bounds__(256) void conv0_ln_gelu_kernel(const float* __restrict__ x, long long n, int L, long long rows, int C, int k, int s,
                                                            const float* __restrict__ W, const float* __restrict__ bias,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ y) {
    const long long row = (long long)blockIdx.x * HB_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const long long b = row / L, t = row - b * L;
    const float* xr = x + b * n + t * s;                   // t s + k <= (L - 1) s + k <= n
    float v[HB_PER_LANE];
#pragma unroll
    for (int i = 0; i < HB_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        float acc = 0.f;
        if (c < C) {
            const float* w = W + (size_t)c * k;
            for (int j = 0; j < k; ++j) acc = fmaf(w[j], xr[j], acc);
            acc += bias[c];
        }
        v[i] = acc;
    }
    hb_ln_store(v, lane, C, gamma, beta, HB_CONV_LN_EPS, 1, y + row * C);
}

int launch_conv0_ln_gelu(const float* x, int B, long long n, int L, int C, int k, int s, const float* W, const float* bias, const float* gamma,
                         const float* beta, float* y, hipStream_t st) {
    DSH_REQUIRE(x && W && bias && gamma && beta && y, "conv0: null pointer");
    DSH_REQUIRE(B >= 1 && L >= 1 && k >= 1 && s >= 1 && C >= 1 && C <= 64 * HB_PER_LANE, "conv0: bad dims");
    DSH_REQUIRE((long long)(L - 1) * s + k <= n, "conv0: the last frame would read behind the signal");
    const long long rows = (long long)B * L;
    DSH_REQUIRE((rows + HB_ROWS_PER_BLOCK - 1) / HB_ROWS_PER_BLOCK < (1ll << 31), "conv0: too many frames");
    hipLaunchKernelGGL(conv0_ln_gelu_kernel, dim3((unsigned)((rows + HB_ROWS_PER_BLOCK - 1) / HB_ROWS_PER_BLOCK)), dim3(256), 0, st, x, n, L, rows, C, k,
                       s, W, bias, gamma, beta, y);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- grouped positional convolution ---------------------------------------------------------------------------------------------------
// conv_gemm_f32_kernel<1, 1> of pose_encoder.hip (64 x 64 tile, four waves, LDS rows padded 128 -> 144 bytes, D[n][m] epilogue) with the A side
// walked tap by tap: K tile kt (32 floats; cg % 32 == 0, so a tile lies inside one tap) of output frame t is
//   h[b, t + tap - pk / 2, g cg + c0 .. c0 + 32],  tap = 32 kt / cg, c0 = 32 kt % cg,
// loaded only when that frame is inside [0, M): outside it zeros are staged (the convolution's zero padding; 0 x NaN would be NaN, and the
// frames next to a clip belong to its neighbours or to nobody).  blockIdx.y = group.
// Ragged (lens != nullptr): batch row b owns lens[b] (clamped to [0, M]) of its M frames; the frames behind are staged as zeros in the same
// way, which is all the dense launch at M = lens[b] does differently, and the outputs behind are 0 (their h is not read either).
struct PosConvArgs {
    const float* H; float* Y; const float* W; const float* bias;
    int rows, M, hidden, cg, pk, nt_m;
    const int* lens;
};
constexpr int PC_LDS_ROW = 144;
constexpr int PC_LDS = 2 * 2 * 64 * PC_LDS_ROW;

__global__ __launch_bounds__(256) void pos_conv_gemm_f32_kernel(PosConvArgs p) {
    constexpr int NTHR = 256, A_LDS = 64 * PC_LDS_ROW, NP = 64 * 8 / NTHR;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int g = blockIdx.y;
    const int nt_n = p.cg / 64 + (p.cg % 64 != 0);
    const int bm = blockIdx.x / nt_n, bn = blockIdx.x % nt_n;
    const int m0 = bm * 64, n0 = bn * 64;
    const int K = p.pk * p.cg, nk = K / 32, half = p.pk / 2;

    const float* a_src[NP];
    const float* w_src[NP];
    int a_t[NP], a_end[NP], lds_off[NP];
    const int c16 = tid & 7;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int row = (tid + i * NTHR) >> 3;
        int ra = m0 + row; ra = ra < p.rows ? ra : p.rows - 1;
        const int b = ra / p.M, t = ra - b * p.M;
        a_src[i] = p.H + (size_t)b * p.M * p.hidden + (size_t)g * p.cg + c16 * 4;
        a_t[i] = t - half;
        a_end[i] = p.M;
        if (p.lens) { const int own = p.lens[b]; a_end[i] = own < 0 ? 0 : (own > p.M ? p.M : own); }
        int rw = n0 + row; rw = rw < p.cg ? rw : p.cg - 1;
        w_src[i] = p.W + ((size_t)g * p.cg + rw) * K + c16 * 4;
        lds_off[i] = row * PC_LDS_ROW + c16 * 16;
    }

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    u32x4 ra[NP], rw[NP];
    auto load_tile = [&](int kt) {
        const int koff = kt * 32, tap = koff / p.cg, c0 = koff - tap * p.cg;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int f = a_t[i] + tap;
            ra[i] = (f >= 0 && f < a_end[i]) ? *reinterpret_cast<const u32x4*>(a_src[i] + (size_t)f * p.hidden + c0) : zero4;
            rw[i] = *reinterpret_cast<const u32x4*>(w_src[i] + koff);
        }
    };
    char* sA = smem;
    char* sW = smem + 2 * A_LDS;
    load_tile(0);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        *reinterpret_cast<u32x4*>(sA + lds_off[i]) = ra[i];
        *reinterpret_cast<u32x4*>(sW + lds_off[i]) = rw[i];
    }
    __syncthreads();

    const int frag_row = lane & 31, frag_kb = (lane >> 5) * 16;
    const int a_frag0 = (wm * 32 + frag_row) * PC_LDS_ROW + frag_kb;
    const int w_frag0 = (wn * 32 + frag_row) * PC_LDS_ROW + frag_kb;
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = (kt + 1) < nk;
        if (more) load_tile(kt + 1);
        const char* cA = sA + cur * A_LDS;
        const char* cW = sW + cur * A_LDS;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            // each lane holds 4 consecutive k and issues 4 MFMAs; the k slots of A and B are permuted identically (see pose_encoder.hip)
            const f32x4 af = *reinterpret_cast<const f32x4*>(cA + a_frag0 + c * 32);
            const f32x4 bf = *reinterpret_cast<const f32x4*>(cW + w_frag0 + c * 32);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bf.x, af.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bf.y, af.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bf.z, af.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bf.w, af.w, acc, 0, 0, 0);
        }
        if (more) {
            char* nA = sA + (cur ^ 1) * A_LDS;
            char* nW = sW + (cur ^ 1) * A_LDS;
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                *reinterpret_cast<u32x4*>(nA + lds_off[i]) = ra[i];
                *reinterpret_cast<u32x4*>(nW + lds_off[i]) = rw[i];
            }
        }
        __syncthreads();
        cur ^= 1;
    }

    // D[n][m]: m = lane & 31, n = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int row = m0 + wm * 32 + (lane & 31);
    if (row >= p.rows) return;
    const size_t base = (size_t)row * p.hidden + (size_t)g * p.cg;
    const bool behind = p.lens && row % p.M >= p.lens[row / p.M];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int col = n0 + wn * 32 + 8 * q + 4 * (lane >> 5);
        if (col >= p.cg) continue;
        if (behind) { *reinterpret_cast<f32x4*>(p.Y + base + col) = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; continue; }
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.bias + g * p.cg + col);
        const f32x4 h4 = *reinterpret_cast<const f32x4*>(p.H + base + col);
        f32x4 o4;
        o4.x = h4.x + gelu_f(acc[4 * q] + b4.x);
        o4.y = h4.y + gelu_f(acc[4 * q + 1] + b4.y);
        o4.z = h4.z + gelu_f(acc[4 * q + 2] + b4.z);
        o4.w = h4.w + gelu_f(acc[4 * q + 3] + b4.w);
        *reinterpret_cast<f32x4*>(p.Y + base + col) = o4;
    }
}

int launch_pos_conv(const float* h, int B, int M, int hidden, int groups, int pk, const float* W, const float* bias, float* h_out, hipStream_t s,
                    const int* lens) {
    DSH_REQUIRE(h && W && bias && h_out && h != h_out, "pos conv: null or aliased tensors");
    DSH_REQUIRE(B >= 1 && M >= 1 && groups >= 1 && hidden % groups == 0 && (hidden / groups) % 32 == 0, "pos conv: channels per group must be a multiple of 32");
    DSH_REQUIRE(pk >= 2 && pk % 2 == 0, "pos conv: the kernel width must be even");
    DSH_REQUIRE((long long)B * M < (1ll << 31) - 64 && groups < 65536, "pos conv: batch too large");
    DSH_REQUIRE(((uintptr_t)h % 16) == 0 && ((uintptr_t)W % 16) == 0 && ((uintptr_t)bias % 16) == 0 && ((uintptr_t)h_out % 16) == 0, "pos conv: 16-byte alignment");
    static bool attr = false;
    if (!attr) {
        DSH_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pos_conv_gemm_f32_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, PC_LDS));
        attr = true;
    }
    PosConvArgs a{h, h_out, W, bias, B * M, M, hidden, hidden / groups, pk, ceil_div(B * M, 64), lens};
    const int nt_n = ceil_div(a.cg, 64);
    hipLaunchKernelGGL(pos_conv_gemm_f32_kernel, dim3((unsigned)(a.nt_m * nt_n), (unsigned)groups), dim3(256), PC_LDS, s, a);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- the network ------------------------------------------------------------------------------------------------------------------------
static const char* const POS = "encoder.pos_conv_embed.conv.";

int HubertEncoder::validate(const HubertConfig& c) {
    DSH_REQUIRE(c.hidden > 0 && c.layers >= 0 && c.heads > 0 && c.intermediate > 0, "dsh_hubert_create: sizes must be positive");
    DSH_REQUIRE(c.hidden == c.heads * 64, "dsh_hubert_create: heads must be 64 wide (hidden / heads == 64)");
    DSH_REQUIRE(c.hidden <= 1024 && c.hidden % 32 == 0 && c.intermediate % 32 == 0, "dsh_hubert_create: hidden <= 1024; hidden and intermediate multiples of 32");
    for (int i = 0; i < 7; ++i) {
        DSH_REQUIRE(c.conv_dim[i] > 0 && c.conv_dim[i] % 32 == 0 && c.conv_dim[i] <= 1024, "dsh_hubert_create: every conv_dim must be a multiple of 32, at most 1024");
        DSH_REQUIRE(c.conv_kernel[i] >= 1 && c.conv_stride[i] >= 1, "dsh_hubert_create: conv kernels and strides must be positive");
    }
    DSH_REQUIRE(c.pos_groups >= 1 && c.hidden % c.pos_groups == 0 && (c.hidden / c.pos_groups) % 32 == 0, "dsh_hubert_create: (hidden / pos_groups) % 32 must be 0");
    DSH_REQUIRE(c.pos_kernel >= 2 && c.pos_kernel % 2 == 0, "dsh_hubert_create: pos_kernel must be even");
    DSH_REQUIRE(c.ln_eps == 1e-5f, "dsh_hubert_create: layer_norm_eps must be 1e-5 (the folded-LayerNorm launch has it built in)");
    return 0;
}

HubertEncoder::HubertEncoder(const HubertConfig& c, hipStream_t s) : cfg_(c), stream_(s) {
    auto add = [&](const std::string& k, std::vector<int64_t> sh) { expected_.emplace_back(k, std::move(sh)); };
    auto lin = [&](const std::string& k, int n, int kk) { add(k + ".weight", {n, kk}); add(k + ".bias", {n}); };
    auto ln = [&](const std::string& k, int n) { add(k + ".weight", {n}); add(k + ".bias", {n}); };
    for (int i = 0; i < 7; ++i) {
        const std::string k = "feature_extractor.conv_layers." + std::to_string(i);
        add(k + ".conv.weight", {c.conv_dim[i], i ? c.conv_dim[i - 1] : 1, c.conv_kernel[i]});
        add(k + ".conv.bias", {c.conv_dim[i]});
        ln(k + ".layer_norm", c.conv_dim[i]);
    }
    ln("feature_projection.layer_norm", c.conv_dim[6]);
    lin("feature_projection.projection", c.hidden, c.conv_dim[6]);
    add(std::string(POS) + "bias", {c.hidden});
    add(std::string(POS) + "weight_g", {1, 1, c.pos_kernel});
    add(std::string(POS) + "weight_v", {c.hidden, c.hidden / c.pos_groups, c.pos_kernel});
    for (int l = 0; l < c.layers; ++l) {
        const std::string k = "encoder.layers." + std::to_string(l);
        for (const char* pj : {"q_proj", "k_proj", "v_proj", "out_proj"}) lin(k + ".attention." + pj, c.hidden, c.hidden);
        ln(k + ".layer_norm", c.hidden);
        lin(k + ".feed_forward.intermediate_dense", c.intermediate, c.hidden);
        lin(k + ".feed_forward.output_dense", c.hidden, c.intermediate);
        ln(k + ".final_layer_norm", c.hidden);
    }
    ln("encoder.layer_norm", c.hidden);
}

void HubertEncoder::release_buffers() {
    for (float** p : {&act_a_, &act_b_, &feat_, &h_, &h2_, &qkv_, &att_, &ffn_, &mom_}) { if (*p) (void)hipFree(*p); *p = nullptr; }
    for (bf16** p : {&qkv16_, &att16_, &ffn16_}) { if (*p) (void)hipFree(*p); *p = nullptr; }
    cap_act_ = cap_rows_ = 0;
}

HubertEncoder::~HubertEncoder() {
    if (stream_ && finalized_) (void)hipStreamSynchronize(stream_);
    release_buffers();
    for (void* p : owned_) (void)hipFree(p);
    if (lens_dev_) (void)hipFree(lens_dev_);
    if (owns_stream_) (void)hipStreamDestroy(stream_);
}

int HubertEncoder::load(const char* name, const float* host, const int64_t* shape, int ndim) {
    DSH_REQUIRE(!finalized_, "dsh_hubert_load_tensor: weights already finalized");
    std::string key(name);
    if (key == "masked_spec_embed" || key.rfind("lm_head.", 0) == 0) return 0;        // not part of the encoder's forward
    // the weight-norm pair in the spelling of torch.nn.utils.parametrizations (current transformers) -> the older weight_g / weight_v
    if (key == std::string(POS) + "parametrizations.weight.original0") key = std::string(POS) + "weight_g";
    else if (key == std::string(POS) + "parametrizations.weight.original1") key = std::string(POS) + "weight_v";
    for (const auto& e : expected_) {
        if (e.first != key) continue;
        bool ok = (size_t)ndim == e.second.size();
        for (int i = 0; ok && i < ndim; ++i) ok = shape[i] == e.second[i];
        if (!ok) {
            std::string want, got;
            for (int64_t v : e.second) want += (want.empty() ? "" : ", ") + std::to_string(v);
            for (int i = 0; i < ndim; ++i) got += (got.empty() ? "" : ", ") + std::to_string(shape[i]);
            set_last_error("invalid argument: dsh_hubert_load_tensor: " + std::string(name) + " has shape [" + got + "], expected [" + want + "]");
            return -1;
        }
        DSH_REQUIRE(host != nullptr, "dsh_hubert_load_tensor: null data");
        HostTensor t;
        size_t n = 1;
        for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
        t.data.assign(host, host + n);
        staged_[key] = std::move(t);
        return 0;
    }
    set_last_error("invalid argument: dsh_hubert_load_tensor: unknown key " + std::string(name));
    return -1;
}

int HubertEncoder::check_complete() const {
    for (const auto& e : expected_)
        if (!staged_.count(e.first)) {
            set_last_error("invalid argument: dsh_hubert_finalize: missing weight " + e.first);
            return -1;
        }
    return 0;
}

// fp64 -> bf16, round to nearest even in ONE step (through fp32 the value would be rounded twice)
static uint16_t bf16_rne_from_f64(double d) {
    if (d == 0.0 || !std::isfinite(d)) return f32_to_bf16((float)d).v;
    int e = std::ilogb(d);                                    // |d| = m 2^e, 1 <= m < 2
    if (e < -126) e = -126;                                   // bf16 subnormals: spacing 2^-133
    const double q = std::nearbyint(std::ldexp(d, 7 - e));    // ties to even in the default rounding mode; |q| <= 256
    return f32_to_bf16((float)std::ldexp(q, e - 7)).v;        // q 2^(e - 7) is a bf16 value (or overflows to inf as fp32 does)
}

int HubertEncoder::set_precision(int p) {
    DSH_REQUIRE(!finalized_, "dsh_hubert_set_precision: only before dsh_hubert_finalize");
    DSH_REQUIRE(p == FP32 || p == BF16, "dsh_hubert_set_precision: 0 (fp32) or 1 (bf16)");
    DSH_REQUIRE(p == FP32 || (cfg_.hidden % 64 == 0 && cfg_.intermediate % 64 == 0), "dsh_hubert_set_precision: bf16 needs hidden and intermediate multiples of 64");
    precision_ = p;
    return 0;
}

// One Linear / convolution in its device form, fp64 on the host.  Folded LayerNorm (the pro 1 convention of dsh_op_gemm_f32_pro):
// W' = gamma (.) W, bias' = b + W beta, c = row sums of W' AS ROUNDED to fp32.
int HubertEncoder::pack(int kind, int layer, int* Nout, int* Kout, std::vector<float>* Wf, std::vector<float>* bf, std::vector<float>* cf,
                        std::vector<uint16_t>* W16) const {
    DSH_REQUIRE(!finalized_, "dsh_hubert: the staged weights were released by dsh_hubert_finalize");
    if (int e = check_complete()) return e;
    const HubertConfig& c = cfg_;
    std::vector<double> W, b;
    int N = 0, K = 0;
    const std::vector<float>*gam = nullptr, *bet = nullptr;
    auto plain = [&](const std::string& k, double scale, size_t row0) {
        const auto &w = T(k + ".weight"), &bb = T(k + ".bias");
        const size_t n = bb.size();
        for (size_t r = 0; r < n; ++r) {
            for (int j = 0; j < K; ++j) W[(row0 + r) * K + j] = scale * (double)w[r * K + j];
            b[row0 + r] = scale * (double)bb[r];
        }
    };
    if (kind == CONV) {
        DSH_REQUIRE(layer >= 0 && layer < 7, "dsh_hubert_debug_packed: conv layer out of range");
        const std::string k = "feature_extractor.conv_layers." + std::to_string(layer) + ".conv";
        const int cin = layer ? c.conv_dim[layer - 1] : 1, ks = c.conv_kernel[layer];
        N = c.conv_dim[layer]; K = ks * cin;
        const auto& w = T(k + ".weight");
        W.resize((size_t)N * K); b.assign(T(k + ".bias").begin(), T(k + ".bias").end());
        for (int n = 0; n < N; ++n)
            for (int ci = 0; ci < cin; ++ci)
                for (int j = 0; j < ks; ++j) W[(size_t)n * K + (size_t)j * cin + ci] = w[((size_t)n * cin + ci) * ks + j];     // tap-major
    } else if (kind == FEAT_PROJ) {
        N = c.hidden; K = c.conv_dim[6];
        W.resize((size_t)N * K); b.resize(N);
        plain("feature_projection.projection", 1.0, 0);
        gam = &T("feature_projection.layer_norm.weight"); bet = &T("feature_projection.layer_norm.bias");
    } else if (kind == POS_CONV) {
        const int cg = c.hidden / c.pos_groups, pk = c.pos_kernel;
        N = c.hidden; K = pk * cg;
        const auto &g = T(std::string(POS) + "weight_g"), &v = T(std::string(POS) + "weight_v");
        std::vector<double> nrm(pk, 0.0);
        for (int o = 0; o < N; ++o)
            for (int i = 0; i < cg; ++i)
                for (int j = 0; j < pk; ++j) { const double x = v[((size_t)o * cg + i) * pk + j]; nrm[j] += x * x; }
        for (int j = 0; j < pk; ++j) nrm[j] = std::sqrt(nrm[j]);
        W.resize((size_t)N * K); b.assign(T(std::string(POS) + "bias").begin(), T(std::string(POS) + "bias").end());
        for (int o = 0; o < N; ++o)
            for (int i = 0; i < cg; ++i)
                for (int j = 0; j < pk; ++j) W[(size_t)o * K + (size_t)j * cg + i] = (double)g[j] * (double)v[((size_t)o * cg + i) * pk + j] / nrm[j];
    } else {
        DSH_REQUIRE(kind >= QKV && kind <= FFN_OUT, "dsh_hubert_debug_packed: unknown kind");
        DSH_REQUIRE(layer >= 0 && layer < c.layers, "dsh_hubert_debug_packed: layer out of range");
        const std::string k = "encoder.layers." + std::to_string(layer);
        if (kind == QKV) {
            N = 3 * c.hidden; K = c.hidden;
            W.resize((size_t)N * K); b.resize(N);
            plain(k + ".attention.q_proj", 0.125, 0);                  // head_dim^-1/2 = 1 / 8, exact
            plain(k + ".attention.k_proj", 1.0, c.hidden);
            plain(k + ".attention.v_proj", 1.0, 2 * (size_t)c.hidden);
            gam = &T(k + ".layer_norm.weight"); bet = &T(k + ".layer_norm.bias");
        } else if (kind == OUT_PROJ) {
            N = K = c.hidden;
            W.resize((size_t)N * K); b.resize(N);
            plain(k + ".attention.out_proj", 1.0, 0);
        } else if (kind == FFN_IN) {
            N = c.intermediate; K = c.hidden;
            W.resize((size_t)N * K); b.resize(N);
            plain(k + ".feed_forward.intermediate_dense", 1.0, 0);
            gam = &T(k + ".final_layer_norm.weight"); bet = &T(k + ".final_layer_norm.bias");
        } else {
            N = c.hidden; K = c.intermediate;
            W.resize((size_t)N * K); b.resize(N);
            plain(k + ".feed_forward.output_dense", 1.0, 0);
        }
    }
    if (gam) {
        for (int n = 0; n < N; ++n) {
            double d = b[n];
            for (int j = 0; j < K; ++j) { d += W[(size_t)n * K + j] * (double)(*bet)[j]; W[(size_t)n * K + j] *= (double)(*gam)[j]; }
            b[n] = d;
        }
    }
    *Nout = N; *Kout = K;
    if (Wf) { Wf->resize(W.size()); for (size_t i = 0; i < W.size(); ++i) (*Wf)[i] = (float)W[i]; }
    if (W16) { W16->resize(W.size()); for (size_t i = 0; i < W.size(); ++i) (*W16)[i] = bf16_rne_from_f64(W[i]); }
    if (bf) { bf->resize(N); for (int n = 0; n < N; ++n) (*bf)[n] = (float)b[n]; }
    if (cf) {
        cf->assign(N, 0.0f);
        if (gam)
            for (int n = 0; n < N; ++n) {
                double s = 0.0;
                for (int j = 0; j < K; ++j) s += (double)(float)W[(size_t)n * K + j];
                (*cf)[n] = (float)s;
            }
    }
    return 0;
}

int HubertEncoder::debug_packed(int kind, int layer, int32_t* dims2, float* W, float* bias, float* fc) const {
    int N, K;
    std::vector<float> wf, bf, cf;
    if (layer_kind_bf16(kind)) {
        std::vector<uint16_t> w16;
        if (int e = pack(kind, layer, &N, &K, nullptr, bias ? &bf : nullptr, nullptr, W ? &w16 : nullptr)) return e;
        wf.resize(w16.size());
        for (size_t i = 0; i < w16.size(); ++i) wf[i] = bf16_to_f32(bf16{w16[i]});
        cf.assign(N, 0.0f);
    } else if (int e = pack(kind, layer, &N, &K, W ? &wf : nullptr, bias ? &bf : nullptr, fc ? &cf : nullptr)) return e;
    if (dims2) { dims2[0] = N; dims2[1] = K; }
    if (W) memcpy(W, wf.data(), wf.size() * sizeof(float));
    if (bias) memcpy(bias, bf.data(), bf.size() * sizeof(float));
    if (fc) memcpy(fc, cf.data(), cf.size() * sizeof(float));
    return 0;
}

int HubertEncoder::upload(int kind, int layer, Lin* out) {
    std::vector<float> wf, bf, cf;
    if (layer_kind_bf16(kind)) {             // bf16 weight and fp32 bias only
        std::vector<uint16_t> w16;
        if (int e = pack(kind, layer, &out->N, &out->K, nullptr, &bf, nullptr, &w16)) return e;
        DSH_HIP_CHECK(hipMalloc((void**)&out->W16, w16.size() * sizeof(uint16_t)));
        owned_.push_back(out->W16);
        DSH_HIP_CHECK(hipMemcpy(out->W16, w16.data(), w16.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        DSH_HIP_CHECK(hipMalloc((void**)&out->b, bf.size() * sizeof(float)));
        owned_.push_back(out->b);
        DSH_HIP_CHECK(hipMemcpy(out->b, bf.data(), bf.size() * sizeof(float), hipMemcpyHostToDevice));
        return 0;
    }
    if (int e = pack(kind, layer, &out->N, &out->K, &wf, &bf, &cf)) return e;
    for (auto pr : {std::make_pair(&out->W, &wf), std::make_pair(&out->b, &bf), std::make_pair(&out->c, &cf)}) {
        DSH_HIP_CHECK(hipMalloc((void**)pr.first, pr.second->size() * sizeof(float)));
        owned_.push_back(*pr.first);
        DSH_HIP_CHECK(hipMemcpy(*pr.first, pr.second->data(), pr.second->size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return 0;
}

int HubertEncoder::upload_ln(const std::string& key, int n, Vec* out) {
    for (auto pr : {std::make_pair(&out->g, key + ".weight"), std::make_pair(&out->b, key + ".bias")}) {
        DSH_HIP_CHECK(hipMalloc((void**)pr.first, (size_t)n * sizeof(float)));
        owned_.push_back(*pr.first);
        DSH_HIP_CHECK(hipMemcpy(*pr.first, T(pr.second).data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    }
    return 0;
}

int HubertEncoder::finalize() {
    DSH_REQUIRE(!finalized_, "dsh_hubert_finalize: weights already finalized");
    if (int e = check_complete()) return e;
    int ndev = 0;
    DSH_HIP_CHECK(hipGetDeviceCount(&ndev));
    DSH_REQUIRE(ndev > 0, "no HIP device visible: this library has no CPU fallback");
    if (stream_ == nullptr) {
        DSH_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamDefault));
        owns_stream_ = true;
    }
    for (int i = 0; i < 7; ++i) {
        if (int e = upload(CONV, i, &conv_[i])) return e;
        if (int e = upload_ln("feature_extractor.conv_layers." + std::to_string(i) + ".layer_norm", cfg_.conv_dim[i], &conv_ln_[i])) return e;
    }
    if (int e = upload(FEAT_PROJ, 0, &feat_proj_)) return e;
    if (int e = upload(POS_CONV, 0, &pos_conv_)) return e;
    layer_.resize(cfg_.layers);
    for (int l = 0; l < cfg_.layers; ++l) {
        if (int e = upload(QKV, l, &layer_[l].qkv)) return e;
        if (int e = upload(OUT_PROJ, l, &layer_[l].out)) return e;
        if (int e = upload(FFN_IN, l, &layer_[l].ffn_in)) return e;
        if (int e = upload(FFN_OUT, l, &layer_[l].ffn_out)) return e;
    }
    if (int e = upload_ln("encoder.layer_norm", cfg_.hidden, &final_ln_)) return e;
    staged_.clear();
    finalized_ = true;
    return 0;
}

int HubertEncoder::receptive_field() const {
    long long rf = 1;
    for (int i = 6; i >= 0; --i) rf = (rf - 1) * cfg_.conv_stride[i] + cfg_.conv_kernel[i];
    return (int)rf;
}

long long HubertEncoder::num_frames(long long n) const {
    long long L = n;
    for (int i = 0; i < 7; ++i) {
        if (L < cfg_.conv_kernel[i]) return -1;
        L = (L - cfg_.conv_kernel[i]) / cfg_.conv_stride[i] + 1;
    }
    return L;
}

int HubertEncoder::reserve(int B, long long n) {
    const int P = B < pass_ ? B : pass_;
    long long L[8];
    L[0] = n;
    for (int i = 0; i < 7; ++i) L[i + 1] = (L[i] - cfg_.conv_kernel[i]) / cfg_.conv_stride[i] + 1;
    long long act = 0;
    for (int i = 0; i < 6; ++i) act = std::max(act, (long long)P * L[i + 1] * cfg_.conv_dim[i]);
    const long long rows = (long long)B * L[7];
    if (act <= cap_act_ && rows <= cap_rows_) return 0;
    DSH_HIP_CHECK(hipStreamSynchronize(stream_));           // (growing waits for launches that still use the old buffers)
    release_buffers();
    DSH_HIP_CHECK(hipMalloc((void**)&act_a_, (size_t)act * sizeof(float)));
    DSH_HIP_CHECK(hipMalloc((void**)&act_b_, (size_t)act * sizeof(float)));
    DSH_HIP_CHECK(hipMalloc((void**)&feat_, (size_t)rows * cfg_.conv_dim[6] * sizeof(float)));
    DSH_HIP_CHECK(hipMalloc((void**)&h_, (size_t)rows * cfg_.hidden * sizeof(float)));
    DSH_HIP_CHECK(hipMalloc((void**)&h2_, (size_t)rows * cfg_.hidden * sizeof(float)));
    if (precision_ == BF16) {
        DSH_HIP_CHECK(hipMalloc((void**)&qkv16_, (size_t)rows * 3 * cfg_.hidden * sizeof(bf16)));
        DSH_HIP_CHECK(hipMalloc((void**)&att16_, (size_t)rows * cfg_.hidden * sizeof(bf16)));
        DSH_HIP_CHECK(hipMalloc((void**)&ffn16_, (size_t)rows * cfg_.intermediate * sizeof(bf16)));
        DSH_HIP_CHECK(hipMalloc((void**)&mom_, (size_t)rows * 2 * sizeof(float)));
    } else {
        DSH_HIP_CHECK(hipMalloc((void**)&qkv_, (size_t)rows * 3 * cfg_.hidden * sizeof(float)));
        DSH_HIP_CHECK(hipMalloc((void**)&att_, (size_t)rows * cfg_.hidden * sizeof(float)));
        DSH_HIP_CHECK(hipMalloc((void**)&ffn_, (size_t)rows * cfg_.intermediate * sizeof(float)));
    }
    cap_act_ = act;
    cap_rows_ = rows;
    return 0;
}

int HubertEncoder::encode(const float* x, int B, long long n, float* out) { return run("dsh_hubert_encode", x, B, n, nullptr, out); }

// Rows padded to n_max samples, row b owning lens_samples[b] (HOST).  What couples the frames of an utterance is the positional convolution and
// the attention; both get the row's frame count num_frames(lens_samples[b]), and so does the last LayerNorm, which writes the zeros.  The
// convolution stack needs none: it is a valid convolution, so frame t < num_frames(n_b) of every layer is computed from samples < n_b alone,
// from the same values in the same order as in a row of n_b samples, and the Linears are per frame.  The frames behind hold whatever the padding
// gives (NaN included) until the positional convolution, which never loads them and leaves zeros.
int HubertEncoder::encode_ragged(const float* x, int B, long long n_max, const int64_t* lens_samples, float* out) {
    DSH_REQUIRE(lens_samples, "dsh_hubert_encode_ragged: null lengths");
    return run("dsh_hubert_encode_ragged", x, B, n_max, lens_samples, out);
}

int HubertEncoder::run(const char* what_c, const float* x, int B, long long n, const int64_t* lens_samples, float* out) {
    const std::string what(what_c);
    DSH_REQUIRE(finalized_, what + ": call dsh_hubert_finalize first");
    DSH_REQUIRE(x && out, what + ": null tensor");
    DSH_REQUIRE(B >= 1, what + ": batch must be positive");
    const long long M = num_frames(n);
    if (M < 1) {
        set_last_error("invalid argument: " + what + ": " + std::to_string(n) + " samples are shorter than the receptive field " +
                       std::to_string(receptive_field()));
        return -1;
    }
    DSH_REQUIRE(n < (1ll << 31) && (long long)B * n < (1ll << 31) * 16 && (long long)B * M < (1ll << 24), what + ": batch too large");
    DSH_REQUIRE(((uintptr_t)out % 16) == 0, what + ": the output must be 16-byte aligned");
    const int* lens = nullptr;
    if (lens_samples) {
        lens_host_.resize(B);
        for (int b = 0; b < B; ++b) {
            const long long nb = lens_samples[b], mb = nb <= n ? num_frames(nb) : -1;
            if (nb > n) {
                set_last_error("invalid argument: " + what + ": row " + std::to_string(b) + " has " + std::to_string(nb) + " samples in rows of " +
                               std::to_string(n));
                return -1;
            }
            if (mb < 1) {
                set_last_error("invalid argument: " + what + ": row " + std::to_string(b) + ": " + std::to_string(nb) +
                               " samples are shorter than the receptive field " + std::to_string(receptive_field()));
                return -1;
            }
            lens_host_[b] = (int32_t)mb;
        }
        if (B > cap_lens_) {
            DSH_HIP_CHECK(hipStreamSynchronize(stream_));
            if (lens_dev_) (void)hipFree(lens_dev_);
            lens_dev_ = nullptr; cap_lens_ = 0;
            DSH_HIP_CHECK(hipMalloc((void**)&lens_dev_, (size_t)B * sizeof(int32_t)));
            cap_lens_ = B;
        }
        // one upload per call, in stream order behind the launches of an earlier call that still read the array; the wait lets the next call
        // reuse the host copy
        DSH_HIP_CHECK(hipMemcpyAsync(lens_dev_, lens_host_.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
        DSH_HIP_CHECK(hipStreamSynchronize(stream_));
        lens = lens_dev_;
    }
    if (int e = reserve(B, n)) return e;
    const HubertConfig& c = cfg_;
    long long L[8];
    L[0] = n;
    for (int i = 0; i < 7; ++i) L[i + 1] = (L[i] - c.conv_kernel[i]) / c.conv_stride[i] + 1;
    const int P = B < pass_ ? B : pass_;

    // 2. the convolution stack, `P` batch rows per pass; the last layer writes its rows of feat_ [B, M, conv_dim[6]]
    for (int b0 = 0; b0 < B; b0 += P) {
        const int nb = B - b0 < P ? B - b0 : P;
        float* bufs[2] = {act_a_, act_b_};
        if (int e = launch_conv0_ln_gelu(x + (size_t)b0 * n, nb, n, (int)L[1], c.conv_dim[0], c.conv_kernel[0], c.conv_stride[0], conv_[0].W, conv_[0].b,
                                         conv_ln_[0].g, conv_ln_[0].b, bufs[0], stream_)) return e;
        for (int i = 1; i < 7; ++i) {
            const float* src = bufs[(i - 1) & 1];
            float* dst = i == 6 ? feat_ + (size_t)b0 * M * c.conv_dim[6] : bufs[i & 1];
            ConvGemmArgs a{};
            a.X = src; a.x_clip = L[i] * c.conv_dim[i - 1]; a.x_step = c.conv_stride[i] * c.conv_dim[i - 1];
            a.W = conv_[i].W; a.ldw = conv_[i].K; a.bias = conv_[i].b;
            a.Y = dst; a.y_clip = L[i + 1] * c.conv_dim[i];
            a.Tout = (int)L[i + 1]; a.M = (int)(nb * L[i + 1]); a.N = c.conv_dim[i]; a.Kreal = conv_[i].K; a.Kp = conv_[i].K;
            if (int e = launch_conv_gemm_f32(a, stream_)) return e;
            if (int e = launch_ln_act_rows(dst, nb * L[i + 1], c.conv_dim[i], conv_ln_[i].g, conv_ln_[i].b, HB_CONV_LN_EPS, 1, dst, stream_)) return e;
        }
    }
    const int R = (int)(B * M);
    auto linear = [&](int pro, const float* in, int ld_in, const Lin& w, int act, const float* res, float* dst) -> int {
        GemmProArgs g{};
        g.pro = pro;
        g.seg[0] = in; g.seg_ld[0] = ld_in;
        for (int i = 0; i < 4; ++i) g.seg_end[i] = w.K / 32;
        g.k_real = w.K;
        g.W = w.W; g.ldw = w.K; g.bias = w.b; g.fc = pro == 1 ? w.c : nullptr;
        g.R = res; g.ldr = w.N;
        g.C = dst; g.ldc = w.N;
        g.M = R; g.N = w.N; g.K = w.K; g.act = act;
        return launch_gemm_f32_pro(g, stream_);
    };
    // 3. feature projection (LayerNorm folded)
    if (int e = linear(1, feat_, c.conv_dim[6], feat_proj_, ACT_NONE, nullptr, h2_)) return e;
    // 4. positional convolution: h_ = h2_ + GELU(posconv(h2_))
    if (int e = launch_pos_conv(h2_, B, (int)M, c.hidden, c.pos_groups, c.pos_kernel, pos_conv_.W, pos_conv_.b, h_, stream_, lens)) return e;
    if (tap_) DSH_HIP_CHECK(hipMemcpyAsync(tap_, h_, (size_t)R * c.hidden * sizeof(float), hipMemcpyDeviceToDevice, stream_));
    // 5. the layers
    // BF16: LayerNorm as (mean, rstd) per row + normalise-then-round in the Linear's staging registers; q|k|v, the attention output and the
    // FFN hidden in bf16; h_ stays fp32 and takes both residual additions in place
    auto linear16 = [&](const void* in, bool in_f32, const Lin& w, int act, float* res_out, bf16* dst16) -> int {
        GemmBf16ProArgs g{};
        g.A = in; g.lda = w.K; g.a_f32 = in_f32 ? 1 : 0; g.mom = in_f32 ? mom_ : nullptr;
        g.W = w.W16; g.bias = w.b; g.R = res_out; g.Cf = res_out; g.Cb = dst16;
        g.M = R; g.N = w.N; g.K = w.K; g.act = act;
        return launch_gemm_bf16_pro(g, stream_);
    };
    for (int l = 0; precision_ == BF16 && l < c.layers; ++l) {
        const Layer& ly = layer_[l];
        if (int e = launch_row_moments(h_, R, c.hidden, c.ln_eps, mom_, stream_)) return e;
        if (int e = linear16(h_, true, ly.qkv, ACT_NONE, nullptr, qkv16_)) return e;
        if (int e = lens ? launch_softmax_attention_bf16_ragged(qkv16_, B, (int)M, c.heads, lens, att16_, stream_)
                         : launch_softmax_attention_bf16(qkv16_, B, (int)M, c.heads, att16_, stream_)) return e;
        if (int e = linear16(att16_, false, ly.out, ACT_NONE, h_, nullptr)) return e;
        if (int e = launch_row_moments(h_, R, c.hidden, c.ln_eps, mom_, stream_)) return e;
        if (int e = linear16(h_, true, ly.ffn_in, ACT_GELU, nullptr, ffn16_)) return e;
        if (int e = linear16(ffn16_, false, ly.ffn_out, ACT_NONE, h_, nullptr)) return e;
    }
    for (int l = 0; precision_ == FP32 && l < c.layers; ++l) {
        const Layer& ly = layer_[l];
        if (int e = linear(1, h_, c.hidden, ly.qkv, ACT_NONE, nullptr, qkv_)) return e;
        if (int e = lens ? launch_softmax_attention_ragged(qkv_, B, (int)M, c.heads, lens, att_, stream_)
                         : launch_softmax_attention(qkv_, B, (int)M, c.heads, att_, stream_)) return e;
        if (int e = linear(0, att_, c.hidden, ly.out, ACT_NONE, h_, h_)) return e;
        if (int e = linear(1, h_, c.hidden, ly.ffn_in, ACT_GELU, nullptr, ffn_)) return e;
        if (int e = linear(0, ffn_, c.intermediate, ly.ffn_out, ACT_NONE, h_, h_)) return e;
    }
    // 6. final LayerNorm
    return launch_ln_act_rows(h_, R, c.hidden, final_ln_.g, final_ln_.b, c.ln_eps, 0, out, stream_, lens, (int)M);
}

}  // namespace dsh
