// Linear of the bf16 HuBERT layers on v_mfma_f32_32x32x16_bf16:  C = act(pro(A) W^T + bias) (+ R)
//
//   pro(A)  A fp32 row-major with (mean, rstd) per row: a = RNE_bf16((x - mean) rstd), formed in the staging registers on the way from HBM to
//           LDS (normalise first, then round: the error of the rounded operand scales with |x - mean|, whatever the row mean is; no normalised
//           copy goes to HBM), or A bf16 row-major, staged as it is.
//   W       bf16 [N, K] row-major.  That IS the packed order: the K tile of a weight row is 128 contiguous bytes, which is what the 16-byte
//           staging loads and the ds_read_b128 fragment reads want (gemm.hip's layout), so the host packer only rounds.
//   epi     + bias (fp32), none or erf-GELU (fp32), + fp32 residual R (may alias an fp32 C: a lane reads the four values it then stores), store
//           fp32 or RNE bf16.
// Tile: (64 MI) x (64 MI), MI in {1, 2}, four waves 2 x 2, each (32 MI) x (32 MI) as MI x MI 32 x 32 accumulators; K tile 64 (128 bytes of bf16
// per row; an fp32 A row contributes 256 bytes = two 16-byte loads per 16-byte LDS chunk).  Staging global -> VGPR -> LDS with rows padded
// 128 -> 144 bytes (conflict-free ds_read_b128 fragment reads), double buffered, the loads of tile k + 1 in flight under the MFMAs of tile k, one
// barrier per K tile: the loop of gemm_nt_kernel<bf16, 1> with the prologue in its staging registers.  The MFMA is issued as (W, A), so that the
// result has the output ROW on the lane and four consecutive columns in registers 4 q .. 4 q + 3: 16-byte (fp32) / 8-byte (bf16) epilogue I/O.
// Every output element has ONE accumulator and K ascending, whatever MI and wherever the row sits in M: no split-K, no atomics.
//
// row_moments_kernel: (mean, rstd) of fp32 rows of up to 1024 channels, one wave per row, two-pass (hubert.hip's hb_ln_store arithmetic), written
// once per row; the Linear's blocks of all N tiles read them (8 bytes per row) instead of recomputing them per N-tile column.
#include "dsh_kernels.h"

namespace dsh {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int GB_LDS_ROW = 144;
constexpr int gb_lds_bytes(int MI) { return 2 * 2 * 64 * MI * GB_LDS_ROW; }        // (A + W) x two stages: 36,864 / 73,728 B

constexpr int RM_ROWS_PER_BLOCK = 4, RM_PER_LANE = 16;

__global__ __launch_bounds__(256) void row_moments_kernel(const float* __restrict__ x, int rows, int C, float eps, float* __restrict__ mom) {
    const int row = blockIdx.x * RM_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (size_t)row * C;
    float v[RM_PER_LANE];
#pragma unroll
    for (int i = 0; i < RM_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < C ? xr[c] : 0.f;
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < RM_PER_LANE; ++i) s += v[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < RM_PER_LANE; ++i) {
        const float d = (lane + 64 * i < C) ? v[i] - mean : 0.f;
        q += d * d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    if (lane == 0) {
        f32x2 m2 = {mean, 1.0f / sqrtf(q / (float)C + eps)};
        *reinterpret_cast<f32x2*>(mom + 2 * (size_t)row) = m2;
    }
}

int launch_row_moments(const float* x, int rows, int C, float eps, float* mom, hipStream_t s) {
    DSH_REQUIRE(x && mom && rows > 0 && C > 0 && C <= 64 * RM_PER_LANE, "row_moments: rows of 1 .. 1024 channels");
    DSH_REQUIRE(((uintptr_t)mom % 8) == 0, "row_moments: the output must be 8-byte aligned");
    hipLaunchKernelGGL(row_moments_kernel, dim3((unsigned)ceil_div(rows, RM_ROWS_PER_BLOCK)), dim3(256), 0, s, x, rows, C, eps, mom);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

template <int MI, bool A_F32>
__global__ __launch_bounds__(256) void gemm_bf16_pro_kernel(GemmBf16ProArgs p) {
    constexpr int NTHR = 256, BM = 64 * MI, BN = 64 * MI, T_LDS = BM * GB_LDS_ROW;
    constexpr int NC = BM * 8 / NTHR;                     // 16-byte LDS chunks per thread and operand
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // the N tiles of one M tile sit in adjacent dispatch slots: the A panel is read from HBM once
    const int bm = blockIdx.x / p.nt_n, bn = blockIdx.x % p.nt_n;
    const int m0 = bm * BM, n0 = bn * BN;
    const int nk = p.K / 64;

    const char* a_src[NC];
    const char* w_src[NC];
    int lds_off[NC];
    float a_mean[NC], a_rstd[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int id = tid + i * NTHR, row = id >> 3, c16 = id & 7;
        int ra = m0 + row; ra = ra < p.M ? ra : p.M - 1;
        int rw = n0 + row; rw = rw < p.N ? rw : p.N - 1;
        a_src[i] = reinterpret_cast<const char*>(p.A) + (size_t)ra * p.lda * (A_F32 ? 4 : 2) + c16 * (A_F32 ? 32 : 16);
        w_src[i] = reinterpret_cast<const char*>(p.W) + (size_t)rw * p.K * 2 + c16 * 16;
        lds_off[i] = row * GB_LDS_ROW + c16 * 16;
        if (A_F32) {
            const f32x2 m2 = *reinterpret_cast<const f32x2*>(p.mom + 2 * (size_t)ra);
            a_mean[i] = m2.x; a_rstd[i] = m2.y;
        }
    }

    f32x16 acc[MI][MI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    f32x4 rf[A_F32 ? NC : 1][2];
    u32x4 ra[A_F32 ? 1 : NC], rw[NC];
    auto load_tile = [&](int kt) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            if (A_F32) {
                const f32x4* src = reinterpret_cast<const f32x4*>(a_src[i] + (size_t)kt * 256);
                rf[i][0] = src[0]; rf[i][1] = src[1];
            } else {
                ra[i] = *reinterpret_cast<const u32x4*>(a_src[i] + (size_t)kt * 128);
            }
            rw[i] = *reinterpret_cast<const u32x4*>(w_src[i] + (size_t)kt * 128);
        }
    };
    auto store_tile = [&](char* sA, char* sW) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            if (A_F32) {
                // normalise, then round: one subtraction and one multiplication in fp32 (rn_*: never contracted with a neighbour), RNE to bf16
                const float mu = a_mean[i], rs = a_rstd[i];
                u32x4 o;
                o.x = pack_bf16_pair(rn_mul(rn_sub(rf[i][0].x, mu), rs), rn_mul(rn_sub(rf[i][0].y, mu), rs));
                o.y = pack_bf16_pair(rn_mul(rn_sub(rf[i][0].z, mu), rs), rn_mul(rn_sub(rf[i][0].w, mu), rs));
                o.z = pack_bf16_pair(rn_mul(rn_sub(rf[i][1].x, mu), rs), rn_mul(rn_sub(rf[i][1].y, mu), rs));
                o.w = pack_bf16_pair(rn_mul(rn_sub(rf[i][1].z, mu), rs), rn_mul(rn_sub(rf[i][1].w, mu), rs));
                *reinterpret_cast<u32x4*>(sA + lds_off[i]) = o;
            } else {
                *reinterpret_cast<u32x4*>(sA + lds_off[i]) = ra[i];
            }
            *reinterpret_cast<u32x4*>(sW + lds_off[i]) = rw[i];
        }
    };
    char* sA = smem;
    char* sW = smem + 2 * T_LDS;
    load_tile(0);
    store_tile(sA, sW);
    __syncthreads();

    const int frag = (lane & 31) * GB_LDS_ROW + (lane >> 5) * 16;
    const int a_frag0 = wm * 32 * MI * GB_LDS_ROW + frag;
    const int w_frag0 = wn * 32 * MI * GB_LDS_ROW + frag;
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = (kt + 1) < nk;
        if (more) load_tile(kt + 1);
        const char* cA = sA + cur * T_LDS;
        const char* cW = sW + cur * T_LDS;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            bf16x8 fa[MI], fb[MI];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                fa[i] = *reinterpret_cast<const bf16x8*>(cA + a_frag0 + i * 32 * GB_LDS_ROW + c * 32);
                fb[i] = *reinterpret_cast<const bf16x8*>(cW + w_frag0 + i * 32 * GB_LDS_ROW + c * 32);
            }
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < MI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        }
        if (more) store_tile(sA + (cur ^ 1) * T_LDS, sW + (cur ^ 1) * T_LDS);
        __syncthreads();
        cur ^= 1;
    }

    // D[n][m]: m = lane & 31, n = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int row = m0 + wm * 32 * MI + i * 32 + (lane & 31);
        if (row >= p.M) continue;
#pragma unroll
        for (int j = 0; j < MI; ++j) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int col = n0 + wn * 32 * MI + j * 32 + 8 * q + 4 * (lane >> 5);
                if (col >= p.N) continue;                 // (N % 64 == 0: a group of four columns is inside N or behind it)
                const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.bias + col);
                float v[4] = {acc[i][j][4 * q] + b4.x, acc[i][j][4 * q + 1] + b4.y, acc[i][j][4 * q + 2] + b4.z, acc[i][j][4 * q + 3] + b4.w};
                if (p.act == ACT_GELU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = gelu_f(v[e]);
                }
                if (p.R) {
                    const f32x4 r4 = *reinterpret_cast<const f32x4*>(p.R + (size_t)row * p.N + col);
                    v[0] += r4.x; v[1] += r4.y; v[2] += r4.z; v[3] += r4.w;
                }
                if (p.Cf) {
                    const f32x4 o4 = {v[0], v[1], v[2], v[3]};
                    *reinterpret_cast<f32x4*>(p.Cf + (size_t)row * p.N + col) = o4;
                } else {
                    const u32x2 o2 = {pack_bf16_pair(v[0], v[1]), pack_bf16_pair(v[2], v[3])};
                    *reinterpret_cast<u32x2*>(p.Cb + (size_t)row * p.N + col) = o2;
                }
            }
        }
    }
}

template <int MI, bool A_F32>
static int launch_gb(const GemmBf16ProArgs& a, hipStream_t s) {
    static bool attr = false;
    if (!attr) {
        DSH_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_bf16_pro_kernel<MI, A_F32>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          gb_lds_bytes(MI)));
        attr = true;
    }
    GemmBf16ProArgs b = a;
    b.nt_n = ceil_div(a.N, 64 * MI);
    const long long blocks = (long long)ceil_div(a.M, 64 * MI) * b.nt_n;
    DSH_REQUIRE(blocks < (1ll << 31), "gemm_bf16_pro: too many tiles");
    hipLaunchKernelGGL((gemm_bf16_pro_kernel<MI, A_F32>), dim3((unsigned)blocks), dim3(256), gb_lds_bytes(MI), s, b);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_gemm_bf16_pro(const GemmBf16ProArgs& a, hipStream_t s) {
    DSH_REQUIRE(a.A && a.W && a.bias && (a.Cf != nullptr) != (a.Cb != nullptr), "gemm_bf16_pro: A, W, bias and exactly one of the two outputs");
    DSH_REQUIRE(a.M >= 1 && a.K >= 64 && a.K % 64 == 0 && a.N >= 64 && a.N % 64 == 0, "gemm_bf16_pro: M >= 1, K and N multiples of 64");
    DSH_REQUIRE(a.lda >= a.K && (a.lda * (a.a_f32 ? 4 : 2)) % 16 == 0, "gemm_bf16_pro: the rows of A must be 16-byte multiples of at least K elements");
    DSH_REQUIRE(!a.a_f32 || a.mom, "gemm_bf16_pro: an fp32 A needs its row moments");
    DSH_REQUIRE(a.act == ACT_NONE || a.act == ACT_GELU, "gemm_bf16_pro: activation none or GELU");
    DSH_REQUIRE(!a.R || a.Cf, "gemm_bf16_pro: the residual goes with the fp32 store");
    DSH_REQUIRE(((uintptr_t)a.A % 16) == 0 && ((uintptr_t)a.W % 16) == 0 && ((uintptr_t)a.bias % 16) == 0 && ((uintptr_t)a.R % 16) == 0 &&
                ((uintptr_t)a.Cf % 16) == 0 && ((uintptr_t)a.Cb % 8) == 0 && ((uintptr_t)a.mom % 8) == 0, "gemm_bf16_pro: operand alignment");
    // 128 x 128 tiles (a quarter of the operand re-reads) where they fill the 256 CUs at least once, 64 x 64 below (more blocks in flight) and
    // for the GELU epilogue, whose erf code runs at two waves per SIMD with the large tile.  Measured at 8000 rows on one MI355X, 64 / 128:
    // q|k|v 126 / 103 us, out_proj 45 / 39 us, output_dense 131 / 104 us, intermediate_dense (GELU) 172 / 181 us.
    // tile = 1 / 2 forces a shape (measurements).  The bits do not depend on the shape.
    int mi = (a.act == ACT_NONE && (long long)ceil_div(a.M, 128) * ceil_div(a.N, 128) >= 256) ? 2 : 1;
    if (a.tile == 1 || a.tile == 2) mi = a.tile;
    if (mi == 2) return a.a_f32 ? launch_gb<2, true>(a, s) : launch_gb<2, false>(a, s);
    return a.a_f32 ? launch_gb<1, true>(a, s) : launch_gb<1, false>(a, s);
}

}  // namespace dsh
