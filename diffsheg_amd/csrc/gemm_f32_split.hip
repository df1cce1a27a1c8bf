// Split-bf16 main loop of the fp32 Linears (precision "bf16x3"; GemmProArgs::mma = 1): the launches of gemm_f32_pro.hip — same fronts (PRO 0 / 1 / 2),
// same epilogue, same arguments — with the product formed on v_mfma_f32_32x32x16_bf16 instead of the exact-fp32 MFMA.
//
//   An fp32 number is written x = hi + lo + r with hi = RNE_bf16(x), lo = RNE_bf16(x - hi) (x - hi is exact in fp32), |r| <= 2^-16 |x|, and the
//   product as three bf16 MFMAs with fp32 accumulation,  a w ~ a_lo w_hi + a_hi w_lo + a_hi w_hi;  what is dropped (a_lo w_lo and the two
//   r terms) is at most 3 x 2^-16 |a w|.
//   W       packed ONCE per weight by launch_split_pack_weight (the one packer: the denoiser calls it at finalisation, the op entry into its
//           scratch): the 128 bytes of a K tile of 32 floats become [hi(k = 0 .. 31) | lo(k = 0 .. 31)], 64 bytes of bf16 each, in place of the
//           32 floats — same row stride, same bytes per launch, and the staging is a plain 16-byte copy into the LDS row.
//   A       split in the staging registers between the global load and the LDS write (v_cvt_pk_bf16_f32, RNE), AFTER the front:
//             PRO 0  the raw rows;
//             PRO 2  normalise -> FiLM -> SiLU (gemm_f32_pro.hip's arithmetic), then split;
//             PRO 1  x - x0 with x0 = the mean of the row's first K tile (the shift of the one-pass moments), then split.  A whole-row offset
//                    would otherwise eat the 2^-16 budget (rows at -200 +- 1.7: the split error scales with |x|, the result with |x - mean|).  The
//                    algebra stays exact:  LN(x) W^T + b = rstd ((x - x0) W'^T - (mean - x0) c) + d.  The K - k_real zero-padded concat
//                    columns are staged as 0 (not as -x0), so the moments need no correction for them.
//   LDS     a row of a stage is [hi 64 B | lo 64 B | 16 B pad]: both planes are read as the ds_read_b128 fragments of gemm_bf16_pro.hip (row =
//           lane & 31, 16 bytes = eight k at (lane >> 5) * 8), conflict-free through the 144-byte row stride.
//   Order   one fp32 accumulator per output element, K ascending in steps of 16; within a step the three products are added in the order
//             (1) a_lo w_hi   (2) a_hi w_lo   (3) a_hi w_hi.
//           No split-K, no atomics: the bits depend neither on the tile shape nor on where a row sits in M (the row moments of PRO 1 / 2 are
//           reduced over the same four staging lanes of a row in both shapes).
// Tile: (64 MI) x (64 MI), MI in {1, 2}, four waves 2 x 2 of MI x MI 32 x 32 accumulators, K tile 32 floats, two LDS stages (36,864 / 73,728 B),
// the loop of gemm_bf16_pro.hip: loads of tile k + 1 in flight under the MFMAs of tile k, one barrier per K tile.  Per K tile and wave at MI = 2:
// 16 ds_read_b128 against 24 MFMAs.  The MFMA is issued as (W, A): the output ROW is on the lane, four consecutive columns in registers.
// The row-moment side channel (stats / stats_out) is not carried by this loop: the launcher refuses it.
#include "dsh_kernels.h"

namespace dsh {

typedef float gs32x16 __attribute__((ext_vector_type(16)));
typedef float gs32x4 __attribute__((ext_vector_type(4)));
typedef short gsbf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t gsu32x4 __attribute__((ext_vector_type(4)));

constexpr int GS_ROW = 144;
constexpr int gs_lds_bytes(int MI) { return 2 * 2 * 64 * MI * GS_ROW; }

// (a, b) -> packed hi pair and packed lo pair, both RNE (v_cvt_pk_bf16_f32); the subtraction is exact and must not be contracted
__device__ __forceinline__ void gs_split2(float a, float b, uint32_t& hi, uint32_t& lo) {
    hi = pack_bf16_pair(a, b);
    lo = pack_bf16_pair(rn_sub(a, __uint_as_float(hi << 16)), rn_sub(b, __uint_as_float(hi & 0xffff0000u)));
}

__device__ __forceinline__ float gs_silu(float x) {
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896340736f));
}

// [N][ldw] fp32 (K whole 32-float tiles) -> the packed operand, same shape in 32-bit words: one thread per pair of columns
__global__ __launch_bounds__(256) void split_pack_weight_kernel(const float* __restrict__ W, int N, int K, int ldw, uint32_t* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int half = K / 2;
    if (idx >= (size_t)N * half) return;
    const int n = (int)(idx / half), j = (int)(idx % half), kt = j >> 4, jj = j & 15;
    const size_t base = (size_t)n * ldw + (size_t)kt * 32;
    const float2 v = *reinterpret_cast<const float2*>(W + base + 2 * jj);
    uint32_t hi, lo;
    gs_split2(v.x, v.y, hi, lo);
    out[base + jj] = hi;
    out[base + 16 + jj] = lo;
}

int launch_split_pack_weight(const float* W, int N, int K, int ldw, uint32_t* out, hipStream_t s) {
    DSH_REQUIRE(W && out && N > 0 && K > 0 && K % 32 == 0 && ldw >= K && ldw % 2 == 0, "split_pack_weight: [N, K] with K whole 32-float tiles");
    DSH_REQUIRE(((uintptr_t)W % 8) == 0 && ((uintptr_t)out % 16) == 0, "split_pack_weight: alignment");
    const size_t pairs = (size_t)N * (K / 2);
    DSH_REQUIRE(pairs < ((size_t)1 << 38), "split_pack_weight: too large");
    hipLaunchKernelGGL(split_pack_weight_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, W, N, K, ldw, out);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

template <int PRO, int MI>
__global__ __launch_bounds__(256) void gemm_f32_split_kernel(GemmProArgs p) {
    constexpr int BM = 64 * MI, T_LDS = BM * GS_ROW;
    constexpr int NP = MI;                                  // A: 32-byte column pairs (8 floats) per thread
    constexpr int NC = 2 * MI;                              // W: 16-byte chunks per thread
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int bm, bn;
    {   // XCD-aware order (gemm_f32_pro.hip): the N tiles of one M tile share an L2
        const int NT = p.nt_n, MT = p.nt_m, bid = blockIdx.x;
        if (MT >= 8) { const int group = bid / (8 * NT), rem = bid % (8 * NT); bm = group * 8 + (rem % 8); bn = rem / 8; }
        else { bm = bid / NT; bn = bid % NT; }
        if (bm >= MT) return;
    }
    const int m0 = bm * BM, n0 = bn * BM;
    const int nk = p.K / 32;
    const int q8 = tid & 3, srow = tid >> 2;                // A staging: columns 8 q8 .. 8 q8 + 7 of rows srow + 64 i

    int arow[NP], a_lds[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int row = srow + 64 * i;
        const int ra = m0 + row;
        arow[i] = ra < p.M ? ra : p.M - 1;
        a_lds[i] = row * GS_ROW + q8 * 16;
    }
    const char* w_src[NC];
    int w_lds[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int id = tid + 256 * i, row = id >> 3, c16 = id & 7;
        int rw = n0 + row; rw = rw < p.N ? rw : p.N - 1;
        w_src[i] = reinterpret_cast<const char*>(p.W) + (size_t)rw * p.ldw * 4 + c16 * 16;
        w_lds[i] = row * GS_ROW + c16 * 16;
    }
    const int e0 = p.seg_end[0], e1 = p.seg_end[1], e2 = p.seg_end[2];
    // the rows of K tile kt: segment and first tile of the segment are block-uniform (two-way selects one after the other)
    auto a_ptr = [&](int kt, int i) -> const gs32x4* {
        const float* sb = p.seg[0]; int sld = p.seg_ld[0], k0 = 0;
        if (PRO == 1) {
            if (kt >= e0) { sb = p.seg[1]; sld = p.seg_ld[1]; k0 = e0; }
            if (kt >= e1) { sb = p.seg[2]; sld = p.seg_ld[2]; k0 = e1; }
            if (kt >= e2) { sb = p.seg[3]; sld = p.seg_ld[3]; k0 = e2; }
        }
        return reinterpret_cast<const gs32x4*>(sb + (size_t)arow[i] * sld + (kt - k0) * 32 + q8 * 8);
    };
    auto sum8 = [](const gs32x4& a, const gs32x4& b) { return ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w)); };
    auto quad = [](float t) { t += __shfl_xor(t, 1, 64); t += __shfl_xor(t, 2, 64); return t; };   // the four staging lanes of a row

    gs32x4 rf[NP][2], rsc[PRO == 2 ? NP : 1][2], rsh[PRO == 2 ? NP : 1][2];
    gsu32x4 rw[NC];
    float x0[NP], s1[NP], s2[NP], mean[NP], rstd[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) { x0[i] = 0.f; s1[i] = 0.f; s2[i] = 0.f; mean[i] = 0.f; rstd[i] = 1.f; }
    const float invP = 1.0f / (float)p.k_real;
    const float* f_src[NP];
    if (PRO == 2) {
        // pass 1: one-pass shifted moments of this block's rows (shift = the mean of the row's first K tile, as gemm_f32_pro.hip)
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const gs32x4* r0 = a_ptr(0, i);
            x0[i] = quad(sum8(r0[0], r0[1])) * (1.0f / 32.0f);
        }
        for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const gs32x4* r = a_ptr(kt, i);
                const gs32x4 u = r[0] - x0[i], v = r[1] - x0[i];
                s1[i] += sum8(u, v);
                s2[i] = fmaf(u.x, u.x, fmaf(u.y, u.y, fmaf(u.z, u.z, fmaf(u.w, u.w, fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, s2[i]))))))));
            }
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const float dm = quad(s1[i]) * invP;
            mean[i] = x0[i] + dm;
            rstd[i] = 1.0f / sqrtf(fmaxf(fmaf(-dm, dm, quad(s2[i]) * invP), 0.f) + 1e-5f);
            const int b = (arow[i] / p.frames) % p.bmod;
            f_src[i] = p.film + (size_t)b * p.film_ld + p.film_off + q8 * 8;
        }
    }

    auto load_tile = [&](int kt) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const gs32x4* r = a_ptr(kt, i);
            rf[i][0] = r[0]; rf[i][1] = r[1];
            if (PRO == 2) {
                const gs32x4* sc = reinterpret_cast<const gs32x4*>(f_src[i] + kt * 32);
                const gs32x4* sh = reinterpret_cast<const gs32x4*>(f_src[i] + p.k_real + kt * 32);
                rsc[i][0] = sc[0]; rsc[i][1] = sc[1]; rsh[i][0] = sh[0]; rsh[i][1] = sh[1];
            }
        }
#pragma unroll
        for (int i = 0; i < NC; ++i) rw[i] = *reinterpret_cast<const gsu32x4*>(w_src[i] + (size_t)kt * 128);
    };
    // front -> split -> LDS (kt: the tile the registers hold)
    auto store_tile = [&](char* sA, char* sW, int kt) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            float v[8] = {rf[i][0].x, rf[i][0].y, rf[i][0].z, rf[i][0].w, rf[i][1].x, rf[i][1].y, rf[i][1].z, rf[i][1].w};
            if (PRO == 1) {
                const int col = kt * 32 + q8 * 8;
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = col + e < p.k_real ? rn_sub(v[e], x0[i]) : 0.f;
                s1[i] += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
#pragma unroll
                for (int e = 7; e >= 0; --e) s2[i] = fmaf(v[e], v[e], s2[i]);
            }
            if (PRO == 2) {
                const float sc[8] = {rsc[i][0].x, rsc[i][0].y, rsc[i][0].z, rsc[i][0].w, rsc[i][1].x, rsc[i][1].y, rsc[i][1].z, rsc[i][1].w};
                const float sh[8] = {rsh[i][0].x, rsh[i][0].y, rsh[i][0].z, rsh[i][0].w, rsh[i][1].x, rsh[i][1].y, rsh[i][1].z, rsh[i][1].w};
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = gs_silu(fmaf((v[e] - mean[i]) * rstd[i], sc[e], sh[e]));
            }
            uint32_t hi[4], lo[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) gs_split2(v[2 * e], v[2 * e + 1], hi[e], lo[e]);
            const gsu32x4 h4 = {hi[0], hi[1], hi[2], hi[3]}, l4 = {lo[0], lo[1], lo[2], lo[3]};
            *reinterpret_cast<gsu32x4*>(sA + a_lds[i]) = h4;
            *reinterpret_cast<gsu32x4*>(sA + a_lds[i] + 64) = l4;
        }
#pragma unroll
        for (int i = 0; i < NC; ++i) *reinterpret_cast<gsu32x4*>(sW + w_lds[i]) = rw[i];
    };

    gs32x16 acc[MI][MI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    char* sA = smem;
    char* sW = smem + 2 * T_LDS;
    load_tile(0);
    if (PRO == 1) {
#pragma unroll
        for (int i = 0; i < NP; ++i) x0[i] = quad(sum8(rf[i][0], rf[i][1])) * (1.0f / 32.0f);
    }
    store_tile(sA, sW, 0);
    __syncthreads();

    const int frag = (lane & 31) * GS_ROW + (lane >> 5) * 16;
    const int a_frag0 = wm * 32 * MI * GS_ROW + frag;
    const int w_frag0 = wn * 32 * MI * GS_ROW + frag;
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = (kt + 1) < nk;
        if (more) load_tile(kt + 1);
        const char* cA = sA + cur * T_LDS;
        const char* cW = sW + cur * T_LDS;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            gsbf16x8 ah[MI], al[MI], wh[MI], wl[MI];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                ah[i] = *reinterpret_cast<const gsbf16x8*>(cA + a_frag0 + i * 32 * GS_ROW + c * 32);
                al[i] = *reinterpret_cast<const gsbf16x8*>(cA + a_frag0 + i * 32 * GS_ROW + c * 32 + 64);
                wh[i] = *reinterpret_cast<const gsbf16x8*>(cW + w_frag0 + i * 32 * GS_ROW + c * 32);
                wl[i] = *reinterpret_cast<const gsbf16x8*>(cW + w_frag0 + i * 32 * GS_ROW + c * 32 + 64);
            }
            // the three products of this k-step in their fixed order; the MI x MI accumulators in between keep dependent MFMAs apart
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < MI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[j], al[i], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < MI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[j], ah[i], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < MI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[j], ah[i], acc[i][j], 0, 0, 0);
        }
        if (more) store_tile(sA + (cur ^ 1) * T_LDS, sW + (cur ^ 1) * T_LDS, kt + 1);
        __syncthreads();
        cur ^= 1;
    }

    float* stat = reinterpret_cast<float*>(smem);               // [BM][2] (mean - x0, rstd); the stages are free behind the last barrier
    if (PRO == 1) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const float dm = quad(s1[i]) * invP;
            const float rs = 1.0f / sqrtf(fmaxf(fmaf(-dm, dm, quad(s2[i]) * invP), 0.f) + 1e-5f);
            if (q8 == 0) { stat[(srow + 64 * i) * 2] = dm; stat[(srow + 64 * i) * 2 + 1] = rs; }
        }
        __syncthreads();
    }

    // ---- epilogue (gemm_f32_pro.hip's): [fold] -> bias -> activation -> (+residual) -> (+row constant) -> store.
    // D[n][m]: m = lane & 31, n = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int rl = wm * 32 * MI + i * 32 + (lane & 31);
        const int row = m0 + rl;
        if (row >= p.M) continue;
        float dm = 0.f, rs = 1.f;
        if (PRO == 1) { dm = stat[rl * 2]; rs = stat[rl * 2 + 1]; }
#pragma unroll
        for (int j = 0; j < MI; ++j) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int col = n0 + wn * 32 * MI + j * 32 + 8 * q + 4 * (lane >> 5);
                if (col >= p.N) continue;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * q + e];
                const gs32x4 b4 = *reinterpret_cast<const gs32x4*>(p.bias + col);
                if (PRO == 1) {
                    const gs32x4 c4 = *reinterpret_cast<const gs32x4*>(p.fc + col);
                    v[0] = fmaf(rs, fmaf(-dm, c4.x, v[0]), b4.x); v[1] = fmaf(rs, fmaf(-dm, c4.y, v[1]), b4.y);
                    v[2] = fmaf(rs, fmaf(-dm, c4.z, v[2]), b4.z); v[3] = fmaf(rs, fmaf(-dm, c4.w, v[3]), b4.w);
                } else {
                    v[0] += b4.x; v[1] += b4.y; v[2] += b4.z; v[3] += b4.w;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = apply_act(v[e], p.act);
                if (p.R) { const gs32x4 r4 = *reinterpret_cast<const gs32x4*>(p.R + (size_t)row * p.ldr + col); v[0] += r4.x; v[1] += r4.y; v[2] += r4.z; v[3] += r4.w; }
                if (p.row_const && row < p.n_const_rows) { const gs32x4 k4 = *reinterpret_cast<const gs32x4*>(p.row_const + col); v[0] += k4.x; v[1] += k4.y; v[2] += k4.z; v[3] += k4.w; }
                const gs32x4 o4 = {v[0], v[1], v[2], v[3]};
                *reinterpret_cast<gs32x4*>(p.C + (size_t)row * p.ldc + col) = o4;
            }
        }
    }
}

template <int PRO, int MI>
static int launch_gs(const GemmProArgs& a, hipStream_t s) {
    static bool attr = false;
    if (!attr) {
        DSH_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_f32_split_kernel<PRO, MI>), hipFuncAttributeMaxDynamicSharedMemorySize, gs_lds_bytes(MI)));
        attr = true;
    }
    GemmProArgs b = a;
    b.nt_n = ceil_div(a.N, 64 * MI);
    b.nt_m = ceil_div(a.M, 64 * MI);
    const long long blocks = b.nt_m >= 8 ? (long long)ceil_div(b.nt_m, 8) * 8 * b.nt_n : (long long)b.nt_m * b.nt_n;
    DSH_REQUIRE(blocks < (1ll << 31), "gemm_f32_pro (split bf16): too many tiles");
    count_launch(LC_GEMM_F32_SPLIT);
    if (MI == 2) count_launch(LC_GEMM_F32_SPLIT_128);
    hipLaunchKernelGGL((gemm_f32_split_kernel<PRO, MI>), dim3((unsigned)blocks), dim3(256), gs_lds_bytes(MI), s, b);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// called by launch_gemm_f32_pro (which has validated the arguments the two loops share) when a.mma == 1; a.W is the PACKED operand
int launch_gemm_f32_split(const GemmProArgs& a, hipStream_t s) {
    DSH_REQUIRE(!a.stats && !a.stats_out, "gemm_f32_pro (split bf16): the row-moment side channel (stats / stats_out) is not carried by the split loop");
    DSH_REQUIRE(a.tile >= 0 && a.tile <= 2, "gemm_f32_pro (split bf16): tile 0 (the launcher picks), 1 (64 x 64) or 2 (128 x 128)");
    for (int i = 0; i < (a.pro == 1 ? 4 : 1); ++i) DSH_REQUIRE(a.seg_ld[i] % 4 == 0, "gemm_f32_pro (split bf16): row strides must be multiples of 4");
    // 128 x 128 tiles (half the L2 -> LDS bytes per FLOP) where they fill the 256 CUs at least once, 64 x 64 below.  tile = 1 / 2 forces a
    // shape (tests, measurements); the bits do not depend on it.
    int mi = (long long)ceil_div(a.M, 128) * ceil_div(a.N, 128) >= 256 ? 2 : 1;
    if (a.tile) mi = a.tile;
    if (mi == 2) return a.pro == 0 ? launch_gs<0, 2>(a, s) : a.pro == 1 ? launch_gs<1, 2>(a, s) : launch_gs<2, 2>(a, s);
    return a.pro == 0 ? launch_gs<0, 1>(a, s) : a.pro == 1 ? launch_gs<1, 1>(a, s) : launch_gs<2, 1>(a, s);
}

}  // namespace dsh
