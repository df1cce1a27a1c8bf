// FGD pose encoder (HalfEmbeddingNet = PoseEncoderConv in eval mode, models/motion_autoencoder.py:38-100,192-204), fp32 on the exact-fp32
// matrix pipe (v_mfma_f32_32x32x2_f32), the path that is inside the project's 1e-3 bar: FGD is a difference of traces of nearly equal
// matrices.
//
// Conv1d as an implicit GEMM without im2col.  Activations are channels-last [B, T, C]; the im2col row of output frame t is then the
// CONTIGUOUS slice x[b, s t : s t + k, :] (k C floats, s = stride), so a conv is the NT product of gemm.hip with overlapping A rows:
//   row m -> (b, t) = (m / T_out, m % T_out),  A row base = b * x_clip + t * s C,  W repacked once to [out, k C] (k-major, channel minor).
// The kernel below is gemm_nt_kernel's fp32 form (same staging, LDS rows padded 128 -> 144 bytes, same fragment trick and D[n][m]
// epilogue; see the top of gemm.hip) with three differences: the A row base above, the K pad, and the output address
// b * y_clip + t * N + n, which lets the last conv write straight into the K-padded rows the first Linear reads (its flattened row IS
// the channels-last conv output; the Linear's columns are permuted at load from the reference's channel-major flatten).
// K pad: K = 3 * 232 = 696 is not a multiple of the 32-float K tile.  The weights are zero padded; on the activation side the 16-byte
// loads whose k >= Kreal are NOT issued and zeros are staged instead (0 x NaN is NaN: the last output row of a clip would otherwise
// read frame n_poses of the caller's tensor, or past its end).  Kreal % 4 == 0, so a 16-byte piece is entirely inside or outside.
// BatchNorm (eval) is folded into weight and bias in fp64 at load; LeakyReLU(0.2) runs in the epilogue.  The `act` of out_net is
// nn.LeakyReLU(True): negative slope 1.0, the identity, so out_net + fc_mu is a chain of plain Linears, run through launch_gemm_f32.
#include <cmath>
#include <cstring>

#include "fgd.h"

namespace dsh {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PE_LDS_ROW = 144;              // one K tile (32 floats, 128 bytes) padded: conflict-free ds_read_b128 fragment reads, as gemm.hip
constexpr int pe_lds_bytes(int MI, int NJ) { return 2 * 32 * (2 * MI + 2 * NJ) * PE_LDS_ROW; }

// Block tile (64 MI) x (64 NJ), 4 waves (2 x 2), each wave MI x NJ accumulators of 32 x 32.
template <int MI, int NJ>
__global__ __launch_bounds__(256) void conv_gemm_f32_kernel(ConvGemmArgs p) {
    constexpr int NTHR = 256;
    constexpr int BM = 64 * MI, BN = 64 * NJ, A_LDS = BM * PE_LDS_ROW, W_LDS = BN * PE_LDS_ROW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // XCD-aware block order of gemm_nt_kernel: the N tiles of one M tile share an XCD (one L2), so the A panel comes from HBM once
    int bm, bn;
    {
        const int NT = p.nt_n, MT = p.nt_m, bid = blockIdx.x;
        if (MT >= 8) {
            const int group = bid / (8 * NT), rem = bid % (8 * NT);
            bm = group * 8 + (rem % 8);
            bn = rem / 8;
        } else {
            bm = bid / NT;
            bn = bid % NT;
        }
        if (bm >= MT) return;
    }
    const int m0 = bm * BM, n0 = bn * BN;
    const int nk = p.Kp / 32;

    constexpr int NA = BM * 8 / NTHR, NW = BN * 8 / NTHR, NMAX = NA > NW ? NA : NW;
    const float* a_src[NA];
    const float* w_src[NW];
    int lds_off[NMAX];
    const int c16 = tid & 7;                              // the same 16-byte column for every piece of this thread (NTHR % 8 == 0)
#pragma unroll
    for (int i = 0; i < NMAX; ++i) {
        const int row = (tid + i * NTHR) >> 3;
        if (i < NA) {
            int ra = m0 + row; ra = ra < p.M ? ra : p.M - 1;
            const int b = ra / p.Tout, t = ra - b * p.Tout;
            a_src[i] = p.X + (size_t)b * p.x_clip + (size_t)t * p.x_step + c16 * 4;
        }
        if (i < NW) { int rw = n0 + row; rw = rw < p.N ? rw : p.N - 1; w_src[i] = p.W + (size_t)rw * p.ldw + c16 * 4; }
        lds_off[i] = row * PE_LDS_ROW + c16 * 16;
    }
    const int k_lane = c16 * 4;                           // first k of this thread's piece inside a K tile

    f32x16 acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    u32x4 ra[NA], rw[NW];
    {
        const bool a_ok = k_lane < p.Kreal;
#pragma unroll
        for (int i = 0; i < NA; ++i) ra[i] = a_ok ? *reinterpret_cast<const u32x4*>(a_src[i]) : zero4;
#pragma unroll
        for (int i = 0; i < NW; ++i) rw[i] = *reinterpret_cast<const u32x4*>(w_src[i]);
    }
    char* sA = smem;
    char* sW = smem + 2 * A_LDS;
#pragma unroll
    for (int i = 0; i < NA; ++i) *reinterpret_cast<u32x4*>(sA + lds_off[i]) = ra[i];
#pragma unroll
    for (int i = 0; i < NW; ++i) *reinterpret_cast<u32x4*>(sW + lds_off[i]) = rw[i];
    __syncthreads();

    const int frag_row = lane & 31;
    const int frag_kb = (lane >> 5) * 16;
    const int a_frag0 = (wm * 32 * MI + frag_row) * PE_LDS_ROW + frag_kb;
    const int w_frag0 = (wn * 32 * NJ + frag_row) * PE_LDS_ROW + frag_kb;

    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = (kt + 1) < nk;
        if (more) {
            const int koff = (kt + 1) * 32;
            const bool a_ok = koff + k_lane < p.Kreal;    // the K pad of the activation side is never read
#pragma unroll
            for (int i = 0; i < NA; ++i) ra[i] = a_ok ? *reinterpret_cast<const u32x4*>(a_src[i] + koff) : zero4;
#pragma unroll
            for (int i = 0; i < NW; ++i) rw[i] = *reinterpret_cast<const u32x4*>(w_src[i] + koff);
        }
        const char* cA = sA + cur * A_LDS;
        const char* cW = sW + cur * W_LDS;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            u32x4 fa[MI], fb[NJ];
#pragma unroll
            for (int i = 0; i < MI; ++i) fa[i] = *reinterpret_cast<const u32x4*>(cA + a_frag0 + i * 32 * PE_LDS_ROW + c * 32);
#pragma unroll
            for (int j = 0; j < NJ; ++j) fb[j] = *reinterpret_cast<const u32x4*>(cW + w_frag0 + j * 32 * PE_LDS_ROW + c * 32);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    // D[n][m]: each lane ends up with 4 consecutive n of one row m -> 16-byte stores.  Each lane holds 4 consecutive k and
                    // issues 4 MFMAs; the k slots of A and B are permuted identically, which leaves the dot product unchanged.
                    const f32x4 af = __builtin_bit_cast(f32x4, fa[i]);
                    const f32x4 bf = __builtin_bit_cast(f32x4, fb[j]);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(bf.x, af.x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(bf.y, af.y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(bf.z, af.z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(bf.w, af.w, acc[i][j], 0, 0, 0);
                }
        }
        if (more) {
            char* nA = sA + (cur ^ 1) * A_LDS;
            char* nW = sW + (cur ^ 1) * W_LDS;
#pragma unroll
            for (int i = 0; i < NA; ++i) *reinterpret_cast<u32x4*>(nA + lds_off[i]) = ra[i];
#pragma unroll
            for (int i = 0; i < NW; ++i) *reinterpret_cast<u32x4*>(nW + lds_off[i]) = rw[i];
        }
        __syncthreads();
        cur ^= 1;
    }

    // epilogue, D[n][m] layout: m = lane & 31, n = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); N % 4 == 0: a quad is inside or outside
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int row = m0 + wm * 32 * MI + i * 32 + (lane & 31);
        if (row >= p.M) continue;
        const int b = row / p.Tout, t = row - b * p.Tout;
        float* yrow = p.Y + (size_t)b * p.y_clip + (size_t)t * p.N;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int col = n0 + wn * 32 * NJ + j * 32 + 8 * q + 4 * (lane >> 5);
                if (col >= p.N) continue;
                const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.bias + col);
                float v[4] = {acc[i][j][4 * q] + b4.x, acc[i][j][4 * q + 1] + b4.y, acc[i][j][4 * q + 2] + b4.z, acc[i][j][4 * q + 3] + b4.w};
                if (p.leaky) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.0f ? v[e] : v[e] * 0.2f;
                }
                f32x4 o4; o4.x = v[0]; o4.y = v[1]; o4.z = v[2]; o4.w = v[3];
                *reinterpret_cast<f32x4*>(yrow + col) = o4;
            }
        }
    }
}

int launch_conv_gemm_f32(const ConvGemmArgs& a, hipStream_t s) {
    DSH_REQUIRE(a.M > 0 && a.N > 0 && a.Kreal > 0 && a.Tout > 0, "conv gemm dims must be positive");
    DSH_REQUIRE(a.Kp % 32 == 0 && a.Kp >= a.Kreal && a.ldw >= a.Kp && a.ldw % 4 == 0, "conv gemm: weights must be padded to the 32-float K tile");
    DSH_REQUIRE(a.Kreal % 4 == 0 && a.x_step % 4 == 0 && a.x_clip % 4 == 0, "conv gemm: activation rows must be 16-byte multiples");
    DSH_REQUIRE(a.N % 4 == 0 && a.y_clip % 4 == 0, "conv gemm: output rows must be 16-byte multiples");
    DSH_REQUIRE(((uintptr_t)a.X % 16) == 0 && ((uintptr_t)a.W % 16) == 0 && ((uintptr_t)a.Y % 16) == 0 && ((uintptr_t)a.bias % 16) == 0,
                "conv gemm operands must be 16-byte aligned");
    // 128 x 64 tiles: N = 300 / 600 is 5 / 10 tiles of 64 columns (6 % padding; 128-wide tiles would waste 22 % at N = 300), and two
    // blocks of 55 KB stay resident per CU.  A few clips only (M < 2048 rows): 64 x 64 tiles, simply more blocks.
    static bool attr = false;
    if (!attr) {
        DSH_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_gemm_f32_kernel<2, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, pe_lds_bytes(2, 1)));
        DSH_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_gemm_f32_kernel<1, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, pe_lds_bytes(1, 1)));
        attr = true;
    }
    ConvGemmArgs b = a;
    const bool big = a.M >= 2048;
    b.nt_n = ceil_div(a.N, 64);
    b.nt_m = ceil_div(a.M, big ? 128 : 64);
    const dim3 grid(b.nt_m >= 8 ? ceil_div(b.nt_m, 8) * 8 * b.nt_n : b.nt_m * b.nt_n);
    if (big) hipLaunchKernelGGL((conv_gemm_f32_kernel<2, 1>), grid, dim3(256), pe_lds_bytes(2, 1), s, b);
    else hipLaunchKernelGGL((conv_gemm_f32_kernel<1, 1>), grid, dim3(256), pe_lds_bytes(1, 1), s, b);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ void stage_clips_kernel(const float* __restrict__ x, int frames, int C, float* __restrict__ y, int n_poses, int Cp, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % Cp);
    const size_t bt = i / Cp;
    const int t = (int)(bt % n_poses);
    const size_t b = bt / n_poses;
    y[i] = c < C ? x[(b * frames + t) * C + c] : 0.0f;
}

int launch_stage_clips(const float* x, int B, int frames, int C, float* y, int n_poses, int Cp, hipStream_t s) {
    const size_t n = (size_t)B * n_poses * Cp;
    hipLaunchKernelGGL(stage_clips_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, frames, C, y, n_poses, Cp, n);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- the network ------------------------------------------------------------------------------------------------------
static const char* const PFX = "pose_encoder.";

FgdEncoder::FgdEncoder(int n_poses, int dim, int base, hipStream_t s) : n_poses_(n_poses), dim_(dim), base_(base), stream_(s) {
    Cp_ = round_up(dim, 4);
    T_[0] = n_poses; T_[1] = n_poses - 2; T_[2] = n_poses - 4; T_[3] = (T_[2] - 4) / 2 + 1; T_[4] = T_[3] - 2;
    auto add = [&](const std::string& k, std::vector<int64_t> sh) { expected_.emplace_back(PFX + k, std::move(sh)); };
    auto bn = [&](const std::string& k, int n) {
        add(k + ".weight", {n}); add(k + ".bias", {n}); add(k + ".running_mean", {n}); add(k + ".running_var", {n});
    };
    const int cin[4] = {dim, base, 2 * base, 2 * base}, cout[4] = {base, 2 * base, 2 * base, base}, ks[4] = {3, 3, 4, 3};
    for (int l = 0; l < 3; ++l) {
        const std::string k = "net." + std::to_string(l);
        add(k + ".0.weight", {cout[l], cin[l], ks[l]}); add(k + ".0.bias", {cout[l]});
        bn(k + ".1", cout[l]);
    }
    add("net.3.weight", {cout[3], cin[3], ks[3]}); add("net.3.bias", {cout[3]});
    // out_net (motion_autoencoder.py:48-83): n_poses 34 starts at the 12 base -> 4 base Linear, every other length has one more in front
    std::vector<int> widths;
    if (n_poses == 34) { widths = {T_[4] * base, 4 * base, 2 * base, base}; lin_idx_ = {0, 3, 6}; bn_idx_ = {1, 4, -1}; }
    else { widths = {T_[4] * base, 12 * base, 4 * base, 2 * base, base}; lin_idx_ = {0, 2, 5, 8}; bn_idx_ = {1, 3, 6, -1}; }
    for (size_t i = 0; i < lin_idx_.size(); ++i) {
        const std::string k = "out_net." + std::to_string(lin_idx_[i]);
        add(k + ".weight", {widths[i + 1], widths[i]}); add(k + ".bias", {widths[i + 1]});
        if (bn_idx_[i] >= 0) bn("out_net." + std::to_string(bn_idx_[i]), widths[i + 1]);
    }
    add("fc_mu.weight", {base, base}); add("fc_mu.bias", {base});
}

void FgdEncoder::release_buffers() {
    if (xs_) (void)hipFree(xs_);
    xs_ = nullptr;
    for (auto& p : act_) { if (p) (void)hipFree(p); p = nullptr; }
    for (auto& p : lbuf_) if (p) (void)hipFree(p);
    lbuf_.clear();
    cap_ = 0;
}

FgdEncoder::~FgdEncoder() {
    if (stream_) (void)hipStreamSynchronize(stream_);
    release_buffers();
    for (auto& l : conv_) { if (l.W) (void)hipFree(l.W); if (l.b) (void)hipFree(l.b); }
    for (auto& l : lin_) { if (l.W) (void)hipFree(l.W); if (l.b) (void)hipFree(l.b); }
    if (owns_stream_) (void)hipStreamDestroy(stream_);
}

static bool ends_with(const std::string& s, const char* suf) {
    const size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

int FgdEncoder::load(const char* name, const float* host, const int64_t* shape, int ndim) {
    DSH_REQUIRE(!finalized_, "dsh_fgd_load_tensor: weights already finalized");
    const std::string key(name);
    // loaded by the reference, unused by HalfEmbeddingNet.forward: accepted and ignored
    if (key.rfind("decoder.", 0) == 0 || key.rfind("pose_encoder.fc_logvar.", 0) == 0 || ends_with(key, ".num_batches_tracked")) return 0;
    for (const auto& e : expected_) {
        if (e.first != key) continue;
        bool ok = (size_t)ndim == e.second.size();
        for (int i = 0; ok && i < ndim; ++i) ok = shape[i] == e.second[i];
        if (!ok) {
            std::string want, got;
            for (int64_t v : e.second) want += (want.empty() ? "" : ", ") + std::to_string(v);
            for (int i = 0; i < ndim; ++i) got += (got.empty() ? "" : ", ") + std::to_string(shape[i]);
            set_last_error("invalid argument: dsh_fgd_load_tensor: " + key + " has shape [" + got + "], expected [" + want + "]");
            return -1;
        }
        DSH_REQUIRE(host != nullptr, "dsh_fgd_load_tensor: null data");
        HostTensor t;
        size_t n = 1;
        for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
        t.data.assign(host, host + n);
        staged_[key] = std::move(t);
        return 0;
    }
    set_last_error("invalid argument: dsh_fgd_load_tensor: unknown key " + key);
    return -1;
}

int FgdEncoder::check_complete() const {
    for (const auto& e : expected_) {
        if (!staged_.count(e.first)) {
            set_last_error("invalid argument: dsh_fgd_finalize: missing weight " + e.first);
            return -1;
        }
    }
    return 0;
}

// Layer `idx` (0 .. 3 the convolutions, then the out_net Linears, fc_mu last) in its device layout, on the host: BatchNorm folded (fp64),
// conv taps repacked, the first Linear's columns permuted, K zero padded to 32 floats.
int FgdEncoder::pack_layer(int idx, Lin* meta, std::vector<float>* wf, std::vector<float>* bf) const {
    DSH_REQUIRE(!finalized_, "dsh_fgd: the staged weights were released by dsh_fgd_finalize");
    DSH_REQUIRE(idx >= 0 && idx < num_layers(), "dsh_fgd: layer index out of range");
    if (int e = check_complete()) return e;
    auto T = [&](const std::string& k) -> const std::vector<float>& { return staged_.at(PFX + k).data; };
    // eval-mode BatchNorm1d (eps 1e-5) behind a conv / Linear: y = (z - mean) g / sqrt(var + eps) + beta, folded in fp64
    auto fold = [&](const std::string& bnk, std::vector<double>& W, std::vector<double>& b, int N, int K) {
        const auto &g = T(bnk + ".weight"), &be = T(bnk + ".bias"), &mu = T(bnk + ".running_mean"), &var = T(bnk + ".running_var");
        for (int n = 0; n < N; ++n) {
            const double sc = (double)g[n] / std::sqrt((double)var[n] + 1e-5);
            for (int k = 0; k < K; ++k) W[(size_t)n * K + k] *= sc;
            b[n] = ((double)b[n] - (double)mu[n]) * sc + (double)be[n];
        }
    };
    std::vector<double> W, b;
    int N = 0, K = 0;
    if (idx < 4) {
        const int l = idx;
        const int cin[4] = {dim_, base_, 2 * base_, 2 * base_}, cinp[4] = {Cp_, base_, 2 * base_, 2 * base_};
        const int cout[4] = {base_, 2 * base_, 2 * base_, base_}, ks[4] = {3, 3, 4, 3};
        const std::string k = l < 3 ? "net." + std::to_string(l) + ".0" : std::string("net.3");
        const auto& w = T(k + ".weight");            // [out, in, ks]
        const auto& bb = T(k + ".bias");
        N = cout[l]; K = ks[l] * cinp[l];
        W.assign((size_t)N * K, 0.0); b.assign(bb.begin(), bb.end());
        // repack to [out, ks, in (padded to 4)]: the k index of the implicit GEMM is (tap, channel), channel minor
        for (int n = 0; n < N; ++n)
            for (int c = 0; c < cin[l]; ++c)
                for (int j = 0; j < ks[l]; ++j) W[(size_t)n * K + (size_t)j * cinp[l] + c] = w[((size_t)n * cin[l] + c) * ks[l] + j];
        if (l < 3) fold("net." + std::to_string(l) + ".1", W, b, N, K);
    } else if (idx - 4 < (int)lin_idx_.size()) {
        const int i = idx - 4;
        const std::string k = "out_net." + std::to_string(lin_idx_[i]);
        const HostTensor& wt = staged_.at(PFX + k + ".weight");
        N = (int)wt.shape[0]; K = (int)wt.shape[1];
        const auto& bb = T(k + ".bias");
        W.resize((size_t)N * K); b.assign(bb.begin(), bb.end());
        if (i == 0) {
            // the reference flattens [B, base, frames] channel-major (column c * frames + t); the conv output here is channels-last
            // (column t * base + c): permute the columns once
            const int F = T_[4];
            for (int n = 0; n < N; ++n)
                for (int c = 0; c < base_; ++c)
                    for (int t = 0; t < F; ++t) W[(size_t)n * K + (size_t)t * base_ + c] = wt.data[(size_t)n * K + (size_t)c * F + t];
        } else {
            for (size_t j = 0; j < W.size(); ++j) W[j] = wt.data[j];
        }
        if (bn_idx_[i] >= 0) fold("out_net." + std::to_string(bn_idx_[i]), W, b, N, K);
    } else {
        const auto& w = T("fc_mu.weight");
        const auto& bb = T("fc_mu.bias");
        N = K = base_;
        W.assign(w.begin(), w.end()); b.assign(bb.begin(), bb.end());
    }
    meta->N = N; meta->Kreal = K; meta->Kp = round_up(K, 32);
    if (wf) {
        wf->assign((size_t)N * meta->Kp, 0.0f);
        for (int n = 0; n < N; ++n)
            for (int k = 0; k < K; ++k) (*wf)[(size_t)n * meta->Kp + k] = (float)W[(size_t)n * K + k];
    }
    if (bf) {
        bf->assign((size_t)round_up(N, 4), 0.0f);
        for (int n = 0; n < N; ++n) (*bf)[n] = (float)b[n];
    }
    return 0;
}

int FgdEncoder::packed_layer(int idx, int32_t* dims3, float* W, float* bias) const {
    Lin m;
    std::vector<float> wf, bf;
    if (int e = pack_layer(idx, &m, W ? &wf : nullptr, bias ? &bf : nullptr)) return e;
    if (dims3) { dims3[0] = m.N; dims3[1] = m.Kreal; dims3[2] = m.Kp; }
    if (W) memcpy(W, wf.data(), wf.size() * sizeof(float));
    if (bias) memcpy(bias, bf.data(), (size_t)m.N * sizeof(float));
    return 0;
}

int FgdEncoder::finalize() {
    DSH_REQUIRE(!finalized_, "dsh_fgd_finalize: weights already finalized");
    if (int e = check_complete()) return e;
    int ndev = 0;
    DSH_HIP_CHECK(hipGetDeviceCount(&ndev));
    DSH_REQUIRE(ndev > 0, "no HIP device visible: this library has no CPU fallback");
    if (stream_ == nullptr) {
        DSH_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamDefault));     // blocking: ordered with the caller's NULL-stream work
        owns_stream_ = true;
    }
    lin_.resize(lin_idx_.size() + 1);
    for (int idx = 0; idx < num_layers(); ++idx) {
        Lin* out = idx < 4 ? &conv_[idx] : &lin_[idx - 4];
        std::vector<float> wf, bf;
        if (int e = pack_layer(idx, out, &wf, &bf)) return e;
        DSH_HIP_CHECK(hipMalloc((void**)&out->W, wf.size() * sizeof(float)));
        DSH_HIP_CHECK(hipMalloc((void**)&out->b, bf.size() * sizeof(float)));
        DSH_HIP_CHECK(hipMemcpy(out->W, wf.data(), wf.size() * sizeof(float), hipMemcpyHostToDevice));
        DSH_HIP_CHECK(hipMemcpy(out->b, bf.data(), bf.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    staged_.clear();
    finalized_ = true;
    return 0;
}

int FgdEncoder::reserve(int batch) {
    if (batch <= cap_) return 0;
    // (growing is rare — the validation batch size is fixed — and has to wait for launches that still use the old buffers)
    DSH_HIP_CHECK(hipStreamSynchronize(stream_));
    release_buffers();
    const int cap = batch;
    auto alloc0 = [&](float** p, size_t n) -> int {
        DSH_HIP_CHECK(hipMalloc((void**)p, n * sizeof(float)));
        DSH_HIP_CHECK(hipMemsetAsync(*p, 0, n * sizeof(float), stream_));   // K-pad columns stay zero: no launch writes them
        return 0;
    };
    if (int e = alloc0(&xs_, (size_t)cap * n_poses_ * Cp_)) return e;
    for (int l = 0; l < 3; ++l)
        if (int e = alloc0(&act_[l], (size_t)cap * T_[l + 1] * conv_[l].N)) return e;
    if (int e = alloc0(&act_[3], (size_t)cap * lin_[0].Kp)) return e;
    lbuf_.assign(lin_.size() - 1, nullptr);
    for (size_t i = 0; i + 1 < lin_.size(); ++i)
        if (int e = alloc0(&lbuf_[i], (size_t)cap * lin_[i + 1].Kp)) return e;
    cap_ = cap;
    return 0;
}

int FgdEncoder::encode(const float* x, int batch, int frames, float* latents) {
    DSH_REQUIRE(finalized_, "dsh_fgd_encode: call dsh_fgd_finalize first");
    DSH_REQUIRE(x && latents, "dsh_fgd_encode: null tensor");
    DSH_REQUIRE(batch > 0, "dsh_fgd_encode: batch must be positive");
    if (frames < n_poses_) {
        set_last_error("invalid argument: dsh_fgd_encode: clips have " + std::to_string(frames) + " frames, the encoder needs n_poses = " +
                       std::to_string(n_poses_));
        return -1;
    }
    DSH_REQUIRE((long long)batch * T_[1] < (1ll << 31), "dsh_fgd_encode: batch too large");
    if (int e = reserve(batch)) return e;
    // net.0 reads the caller's tensor in place (first n_poses frames of every clip) when 16-byte loads can address it
    const float* x0 = x;
    long long x_clip = (long long)frames * dim_;
    if (dim_ % 4 != 0 || ((uintptr_t)x % 16) != 0) {
        if (int e = launch_stage_clips(x, batch, frames, dim_, xs_, n_poses_, Cp_, stream_)) return e;
        x0 = xs_; x_clip = (long long)n_poses_ * Cp_;
    }
    const int cinp[4] = {Cp_, base_, 2 * base_, 2 * base_}, st[4] = {1, 1, 2, 1};
    for (int l = 0; l < 4; ++l) {
        ConvGemmArgs a{};
        a.X = l == 0 ? x0 : act_[l - 1];
        a.x_clip = l == 0 ? x_clip : (long long)T_[l] * cinp[l];
        a.x_step = st[l] * cinp[l];
        a.W = conv_[l].W; a.ldw = conv_[l].Kp; a.bias = conv_[l].b;
        a.Y = act_[l];
        a.y_clip = l == 3 ? (long long)lin_[0].Kp : (long long)T_[l + 1] * conv_[l].N;
        a.Tout = T_[l + 1]; a.M = batch * T_[l + 1]; a.N = conv_[l].N; a.Kreal = conv_[l].Kreal; a.Kp = conv_[l].Kp;
        a.leaky = l < 3;
        if (int e = launch_conv_gemm_f32(a, stream_)) return e;
    }
    // out_net + fc_mu: plain Linears (BatchNorm folded, LeakyReLU(True) is the identity) through the project's fp32 GEMM
    const float* in = act_[3];
    for (size_t i = 0; i < lin_.size(); ++i) {
        const bool last = i + 1 == lin_.size();
        GemmArgs g{};
        g.A = in; g.lda = lin_[i].Kp; g.W = lin_[i].W; g.ldw = lin_[i].Kp; g.bias = lin_[i].b;
        g.Cf = last ? latents : lbuf_[i]; g.ldcf = last ? lin_[i].N : lin_[i + 1].Kp;
        g.M = batch; g.N = lin_[i].N; g.K = lin_[i].Kp;
        if (int e = launch_gemm_f32(g, stream_)) return e;
        in = g.Cf;
    }
    return 0;
}

}  // namespace dsh
