// Row-wise (per-token) kernels of the DiffSHEG denoiser: one 64-lane wavefront owns one token row,
// loads are lane-strided (coalesced 256 B per wave instruction), statistics are wavefront
// reductions in fp32 regardless of the storage type.
//
//   ln_rows            sa_block.norm, with the CFG-null feat_proj constant folded in
//                      (models/transformer.py:119-125, :326-338)
//   ln_film_silu_rows  StylizationBlock: SiLU(LN(y)*(1+scale)+shift)        (:86-97)
//   concat_ln_rows     feat_proj.0 LayerNorm over the un-materialised concat (:304-312, :284-285)
//   im2col3_rows       Conv1d(k=3,p=1) patches for hubert_encoder           (:437-442)
//   temb_rows          timestep_embedding                                    (:42-59)
//   pack_cols          split x into gesture|expression operands              (:741)
//   cfg_mix            classifier-free mix + expression x0                   (:585-586, :717-724)
//   cfg_mix_sched      the same under a guidance schedule: gain per timestep and encoder, then
//   cfg_rescale        the std rescale of the guided eps per clip (no counterpart in the reference)
#include <algorithm>

#include "dsh_common.h"
#include "dsh_kernels.h"

namespace dsh {

constexpr int ROWS_PER_BLOCK = 4;   // 4 waves / block
constexpr int MAX_PER_LANE = 16;    // supports D <= 1024

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void ln_rows_kernel(float* h, int ldh, int M, int D, const float* pre_add,
                                                      int n_pre_rows, const float* gamma, const float* beta,
                                                      T* out, int ldo) {
    const int row = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= M) return;
    float* hr = h + (size_t)row * ldh;
    const bool add = pre_add != nullptr && row < n_pre_rows;
    float v[MAX_PER_LANE];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAX_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        float x = 0.f;
        if (c < D) {
            x = hr[c];
            if (add) { x += pre_add[c]; hr[c] = x; }
        }
        v[i] = x;
        s += x;
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAX_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        const float d = (c < D) ? v[i] - mean : 0.f;
        q += d * d;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + 1e-5f);
    T* orow = out + (size_t)row * ldo;
#pragma unroll
    for (int i = 0; i < MAX_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        if (c < D) orow[c] = from_f32<T>((v[i] - mean) * rstd * gamma[c] + beta[c]);
    }
}

template <typename T>
int launch_ln_rows(float* h, int ldh, int M, int D, const float* pre_add, int n_pre_rows, const float* gamma,
                   const float* beta, T* out, int ldo, hipStream_t s) {
    DSH_REQUIRE(D <= 64 * MAX_PER_LANE, "ln_rows: D too large");
    hipLaunchKernelGGL(ln_rows_kernel<T>, dim3(ceil_div(M, ROWS_PER_BLOCK)), dim3(256), 0, s, h, ldh, M, D, pre_add,
                       n_pre_rows, gamma, beta, out, ldo);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}
template int launch_ln_rows<float>(float*, int, int, int, const float*, int, const float*, const float*, float*, int, hipStream_t);
template int launch_ln_rows<bf16>(float*, int, int, int, const float*, int, const float*, const float*, bf16*, int, hipStream_t);

// ------------------------------------------------------------------------------------------------
template <typename TI, typename T>
__global__ __launch_bounds__(256) void ln_film_silu_rows_kernel(const TI* y, int ldy, int M, int D, const float* gamma,
                                                                const float* beta, const float* film, int film_ld,
                                                                int film_off, int frames, int bmod, T* out, int ldo) {
    const int row = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= M) return;
    const TI* yr = y + (size_t)row * ldy;
    float v[MAX_PER_LANE];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAX_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        const float x = (c < D) ? to_f32<TI>(yr[c]) : 0.f;
        v[i] = x;
        s += x;
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAX_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        const float d = (c < D) ? v[i] - mean : 0.f;
        q += d * d;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + 1e-5f);
    const int b = (row / frames) % bmod;
    const float* fs = film + (size_t)b * film_ld + film_off;   // [scale(D) | shift(D)]
    T* orow = out + (size_t)row * ldo;
#pragma unroll
    for (int i = 0; i < MAX_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        if (c < D) {
            const float n = (v[i] - mean) * rstd * gamma[c] + beta[c];
            orow[c] = from_f32<T>(silu_f(n * (1.0f + fs[c]) + fs[D + c]));
        }
    }
}

template <typename TI, typename T>
int launch_ln_film_silu_rows(const TI* y, int ldy, int M, int D, const float* gamma, const float* beta,
                             const float* film, int film_ld, int film_off, int frames, int bmod, T* out, int ldo,
                             hipStream_t s) {
    DSH_REQUIRE(D <= 64 * MAX_PER_LANE, "ln_film_silu_rows: D too large");
    hipLaunchKernelGGL((ln_film_silu_rows_kernel<TI, T>), dim3(ceil_div(M, ROWS_PER_BLOCK)), dim3(256), 0, s, y, ldy, M,
                       D, gamma, beta, film, film_ld, film_off, frames, bmod, out, ldo);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}
template int launch_ln_film_silu_rows<float, float>(const float*, int, int, int, const float*, const float*, const float*, int, int, int, int, float*, int, hipStream_t);
template int launch_ln_film_silu_rows<float, bf16>(const float*, int, int, int, const float*, const float*, const float*, int, int, int, int, bf16*, int, hipStream_t);
template int launch_ln_film_silu_rows<bf16, bf16>(const bf16*, int, int, int, const float*, const float*, const float*, int, int, int, int, bf16*, int, hipStream_t);

// ------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ float seg_load(const ConcatSegs& sg, int c, int row) {
    // segments are laid out back to back in the virtual concat row
    if (c < sg.w0) return sg.p0[(size_t)row * sg.ld0 + c];                       // latent h (fp32)
    c -= sg.w0;
    if (c < sg.w1) return to_f32<T>(reinterpret_cast<const T*>(sg.p1)[(size_t)row * sg.ld1 + c]);
    c -= sg.w1;
    if (c < sg.w2) return to_f32<T>(reinterpret_cast<const T*>(sg.p2)[(size_t)row * sg.ld2 + c]);
    c -= sg.w2;
    return sg.p3[(size_t)row * sg.ld3 + c];                                       // expr_x0 (fp32)
}

template <typename T>
__global__ __launch_bounds__(256) void concat_ln_rows_kernel(ConcatSegs sg, int M, const float* gamma, const float* beta,
                                                             T* out, int ldo, int Ppad) {
    const int row = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= M) return;
    const int P = sg.w0 + sg.w1 + sg.w2 + sg.w3;
    float v[MAX_PER_LANE];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAX_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        const float x = (c < P) ? seg_load<T>(sg, c, row) : 0.f;
        v[i] = x;
        s += x;
    }
    const float mean = wave_sum(s) / (float)P;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAX_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        const float d = (c < P) ? v[i] - mean : 0.f;
        q += d * d;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)P + 1e-5f);
    T* orow = out + (size_t)row * ldo;
#pragma unroll
    for (int i = 0; i < MAX_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        if (c < P) orow[c] = from_f32<T>((v[i] - mean) * rstd * gamma[c] + beta[c]);
        else if (c < Ppad) orow[c] = from_f32<T>(0.f);
    }
}

template <typename T>
int launch_concat_ln_rows(const ConcatSegs& sg, int M, const float* gamma, const float* beta, T* out, int ldo, int Ppad,
                          hipStream_t s) {
    DSH_REQUIRE(Ppad <= 64 * MAX_PER_LANE, "concat_ln_rows: concat width too large");
    hipLaunchKernelGGL(concat_ln_rows_kernel<T>, dim3(ceil_div(M, ROWS_PER_BLOCK)), dim3(256), 0, s, sg, M, gamma, beta,
                       out, ldo, Ppad);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}
template int launch_concat_ln_rows<float>(const ConcatSegs&, int, const float*, const float*, float*, int, int, hipStream_t);
template int launch_concat_ln_rows<bf16>(const ConcatSegs&, int, const float*, const float*, bf16*, int, int, hipStream_t);

// ------------------------------------------------------------------------------------------------
// out[(b,t), tap*Cin + c] = x[b, t + tap - 1, c]  (zero outside the window: padding=1 per sample)
// lens (nullable): clip b of the padded batch ends at frame lens[b] — source frames beyond it read as zero (by selection, whatever they hold),
// which is the zero padding the clip's convolution sees when it is run alone at that length
template <typename TI, typename T>
__global__ void im2col3_rows_kernel(const TI* x, int ldx, int B, int frames, int Cin, T* out, int ldo, const int* lens) {
    const int row = blockIdx.x;
    const int b = row / frames, t = row % frames;
    const int len = lens ? lens[b] : frames;
    T* orow = out + (size_t)row * ldo;
    for (int tap = 0; tap < 3; ++tap) {
        const int ts = t + tap - 1;
        const bool ok = ts >= 0 && ts < len;
        const TI* xr = x + ((size_t)b * frames + (ok ? ts : 0)) * ldx;
        for (int c = threadIdx.x; c < Cin; c += blockDim.x)
            orow[tap * Cin + c] = ok ? from_f32<T>(to_f32<TI>(xr[c])) : from_f32<T>(0.f);
    }
}

template <typename TI, typename T>
int launch_im2col3_rows(const TI* x, int ldx, int B, int frames, int Cin, T* out, int ldo, hipStream_t s, const int* lens) {
    hipLaunchKernelGGL((im2col3_rows_kernel<TI, T>), dim3(B * frames), dim3(256), 0, s, x, ldx, B, frames, Cin, out, ldo, lens);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}
template int launch_im2col3_rows<float, float>(const float*, int, int, int, int, float*, int, hipStream_t, const int*);
template int launch_im2col3_rows<float, bf16>(const float*, int, int, int, int, bf16*, int, hipStream_t, const int*);
template int launch_im2col3_rows<bf16, bf16>(const bf16*, int, int, int, int, bf16*, int, hipStream_t, const int*);

// ------------------------------------------------------------------------------------------------
// temb[b, j] = cos(t_b f_j) (j < half), sin(t_b f_{j-half}) (j >= half); f_j = exp(-ln(1e4) j / half)
template <typename T>
__global__ void temb_rows_kernel(const int64_t* t, int B, int dim, T* out, int ldo) {
    const int b = blockIdx.x;
    const int half = dim / 2;
    const float tv = (float)t[b];
    for (int j = threadIdx.x; j < half; j += blockDim.x) {
        // the reference builds freqs in fp32: exp(-log(10000) * arange(half) / half)
        const float f = expf(-9.210340371976184f * (float)j / (float)half);
        const float a = tv * f;
        out[(size_t)b * ldo + j] = from_f32<T>(cosf(a));
        out[(size_t)b * ldo + half + j] = from_f32<T>(sinf(a));
    }
}
template <typename T>
int launch_temb_rows(const int64_t* t, int B, int dim, T* out, int ldo, hipStream_t s) {
    hipLaunchKernelGGL(temb_rows_kernel<T>, dim3(B), dim3(256), 0, s, t, B, dim, out, ldo);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}
template int launch_temb_rows<float>(const int64_t*, int, int, float*, int, hipStream_t);
template int launch_temb_rows<bf16>(const int64_t*, int, int, bf16*, int, hipStream_t);

// ------------------------------------------------------------------------------------------------
// out[r, c] = scale * x[r, c0 + c] for c < w, 0 for w <= c < wpad; optional fp32 copy (same scale)
template <typename T>
__global__ void pack_cols_kernel(const float* x, int ldx, int M, int c0, int w, int wpad, float scale, T* out, int ldo,
                                 float* outf, int ldof) {
    const int row = blockIdx.x;
    for (int c = threadIdx.x; c < wpad; c += blockDim.x) {
        const float v = (c < w) ? scale * x[(size_t)row * ldx + c0 + c] : 0.f;
        if (out) out[(size_t)row * ldo + c] = from_f32<T>(v);
        if (outf && c < w) outf[(size_t)row * ldof + c] = v;
    }
}
template <typename T>
int launch_pack_cols(const float* x, int ldx, int M, int c0, int w, int wpad, float scale, T* out, int ldo, float* outf,
                     int ldof, hipStream_t s) {
    hipLaunchKernelGGL(pack_cols_kernel<T>, dim3(M), dim3(128), 0, s, x, ldx, M, c0, w, wpad, scale, out, ldo, outf, ldof);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}
template int launch_pack_cols<float>(const float*, int, int, int, int, int, float, float*, int, float*, int, hipStream_t);
template int launch_pack_cols<bf16>(const float*, int, int, int, int, int, float, bf16*, int, float*, int, hipStream_t);

// ------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------
// eps[b,t,c0+c] = o_u + s_b (o_c - o_u)   (o rows: [0,Mc) unconditional, [cond_row0, cond_row0+Mc) conditional; has_null==0: copy)
// s_b = scale[b * scale_row] (device: read when the kernel runs, so a captured graph follows the context's guidance buffer); a clip whose
// scale is exactly 1 takes o_c itself (u + 1 (k - u) is not k in fp32)
// x0[r,c] = c1[b] * x[b,t,c0+c] - c2[b] * eps   (optional; expression branch feeding the gesture concat)
__global__ void cfg_mix_kernel(const float* o, int ldo, int cond_row0, int frames, int w, int has_null, const float* scale, int scale_row,
                               float* eps, int lde, int c0, const float* x, int ldx, const float* c1, const float* c2,
                               float* x0, int ldx0) {
    const int row = blockIdx.x;
    const int b = row / frames;
    for (int c = threadIdx.x; c < w; c += blockDim.x) {
        float e;
        if (has_null) {
            const float u = o[(size_t)row * ldo + c];
            const float k = o[(size_t)(row + cond_row0) * ldo + c];
            // (the scale is read behind the two loads, not hoisted in front of them: its latency overlaps theirs)
            asm volatile("" ::: "memory");
            const float cs = scale[(size_t)b * scale_row];
            e = cs == 1.0f ? k : rn_add(u, rn_mul(cs, rn_sub(k, u)));
        } else {
            e = o[(size_t)row * ldo + c];
        }
        eps[(size_t)row * lde + c0 + c] = e;
        if (x0) {
            const float a = rn_mul(c1[b], x[(size_t)row * ldx + c0 + c]);
            const float bb = rn_mul(c2[b], e);
            x0[(size_t)row * ldx0 + c] = rn_sub(a, bb);
        }
    }
}
int launch_cfg_mix(const float* o, int ldo, int Mc, int cond_row0, int frames, int w, int has_null, const float* scale, int scale_row,
                   float* eps, int lde, int c0, const float* x, int ldx, const float* c1, const float* c2, float* x0,
                   int ldx0, hipStream_t s) {
    DSH_REQUIRE(!has_null || scale, "cfg_mix: a doubled batch needs its guidance scales");
    hipLaunchKernelGGL(cfg_mix_kernel, dim3(Mc), dim3(128), 0, s, o, ldo, cond_row0, frames, w, has_null, scale, scale_row, eps, lde,
                       c0, x, ldx, c1, c2, x0, ldx0);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Guidance schedule (dsh_set_guidance_schedule): the mix above with the clip's scale shaped per model timestep and encoder, and the
// optional std rescale of the guided prediction.  sched = [gain_expression[n] | gain_gesture[n] | phi_expression, phi_gesture] (device).
//   s_eff = g == 1 ? s : 1 + g (s - 1)   with g = sched[m n + clamp(t_b, 0, n - 1)], s = scale[b scale_row]   (fp32, each op rounded)
//   e     = s_eff == 1 ? k : u + s_eff (k - u)
__device__ __forceinline__ float cfg_sched_scale(const float* scale, int scale_row, const int64_t* t, int t_row, const float* sched, int n,
                                                 int m, int b) {
    const float s = scale[(size_t)b * scale_row];
    int64_t tb = t[(size_t)b * t_row];
    tb = tb < 0 ? 0 : (tb > n - 1 ? n - 1 : tb);               // (never outside the table)
    const float g = sched[(size_t)m * n + tb];
    return g == 1.0f ? s : rn_add(1.0f, rn_mul(g, rn_sub(s, 1.0f)));
}
// two fp64 values per thread summed over the 128 threads of a block in one fixed order (an xor butterfly inside each wave — commutative
// pairs, so every lane holds the same bits — then wave 0 + wave 1); every thread gets both sums.  sh: 4 doubles.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ void block128_sum2(double& a, double& b, double* sh) {
    a = wave_sum_f64(a); b = wave_sum_f64(b);
    const int wv = threadIdx.x >> 6;
    __syncthreads();                                                    // (sh may still be read from the call before)
    if ((threadIdx.x & 63) == 0) { sh[wv] = a; sh[2 + wv] = b; }
    __syncthreads();
    a = sh[0] + sh[1]; b = sh[2] + sh[3];
}
// One block per token row of a doubled batch.  STATS false: the only launch of the encoder, the plain mix with the scale looked up (writes eps
// and the optional x0).  STATS true (phi > 0): writes the un-rescaled e into eps and the row's moments of k and e over its w columns —
// part[row] = {mean k, M2 k, mean e, M2 e} in fp64, M2 = sum (v - mean)^2 taken in a second pass, so a constant row gives exactly 0 — for the
// rows t < len_b only; x0 is left to cfg_rescale_kernel.  (Moments instead of raw power sums: sum v^2 - (sum v)^2 / n leaves a rounding
// residue where the variance is 0.)
template <bool STATS>
__global__ void cfg_mix_sched_kernel(const float* o, int ldo, int cond_row0, int frames, int w, const float* scale, int scale_row,
                                     const int64_t* t, int t_row, const float* sched, int n_steps, int m, const int* lens, float* eps,
                                     int lde, int c0, const float* x, int ldx, const float* c1, const float* c2, float* x0, int ldx0,
                                     double* part) {
    __shared__ double sh[4];
    const int row = blockIdx.x;
    const int b = row / frames;
    double sk = 0.0, se = 0.0;
    for (int c = threadIdx.x; c < w; c += blockDim.x) {
        const float u = o[(size_t)row * ldo + c];
        const float k = o[(size_t)(row + cond_row0) * ldo + c];
        // (scale, timestep and gain are read behind the two loads, as cfg_mix_kernel reads its scale: their latency overlaps the loads')
        asm volatile("" ::: "memory");
        const float cs = cfg_sched_scale(scale, scale_row, t, t_row, sched, n_steps, m, b);
        const float e = cs == 1.0f ? k : rn_add(u, rn_mul(cs, rn_sub(k, u)));
        eps[(size_t)row * lde + c0 + c] = e;
        if (STATS) {
            sk += (double)k; se += (double)e;
        } else if (x0) {
            const float a = rn_mul(c1[b], x[(size_t)row * ldx + c0 + c]);
            const float bb = rn_mul(c2[b], e);
            x0[(size_t)row * ldx0 + c] = rn_sub(a, bb);
        }
    }
    if (!STATS) return;
    const int len = lens ? min(max(lens[b], 0), frames) : frames;
    if (row - b * frames >= len) return;                                 // (block-uniform; padded rows are never read into the moments)
    block128_sum2(sk, se, sh);
    const double mk = sk / (double)w, me = se / (double)w;
    double qk = 0.0, qe = 0.0;
    for (int c = threadIdx.x; c < w; c += blockDim.x) {
        // (k again from o; e as this very thread stored it)
        const double dk = (double)o[(size_t)(row + cond_row0) * ldo + c] - mk, de = (double)eps[(size_t)row * lde + c0 + c] - me;
        qk += dk * dk; qe += de * de;
    }
    block128_sum2(qk, qe, sh);
    if (threadIdx.x == 0) { double* p = part + (size_t)row * 4; p[0] = mk; p[1] = qk; p[2] = me; p[3] = qe; }
}
// Second launch of a rescaled encoder (phi > 0), one block of 128 threads per CFG_RESCALE_ROWS token rows of a clip (a block per row re-read
// the clip's moments 88 times over; a block per clip left 950 blocks walking 11 352 elements each).  Every block of a clip combines the
// clip's <= frames row moments from L2 in one fixed order (thread i takes rows i, i + 128, ... in turn, then block128_sum2: the same f in
// every row of the clip, whatever the batch).  The rows hold w elements each, so the clip's mean is the mean of the row means and its M2 = sum M2_r +
// w sum (mean_r - mean)^2 — exactly 0 for a constant clip.  f = float(phi sigma_k / sigma_e + (1 - phi)) in fp64 with the unbiased deviations
// over the n = len_b w valid elements (f = 1 exactly where s_eff = 1, n < 2, or sigma_e is not finite and positive); the block then scales
// its rows of eps in place (padded rows too: unspecified values stay unspecified) and writes the x0 the single-launch form writes.
constexpr int CFG_RESCALE_ROWS = 8;
__global__ void cfg_rescale_kernel(const double* part, int frames, int w, const float* scale, int scale_row, const int64_t* t, int t_row,
                                   const float* sched, int n_steps, int m, const int* lens, float* eps, int lde, int c0, const float* x,
                                   int ldx, const float* c1, const float* c2, float* x0, int ldx0) {
    __shared__ double sh[4];
    const int nchunk = (frames + CFG_RESCALE_ROWS - 1) / CFG_RESCALE_ROWS, tid = threadIdx.x;
    const int b = blockIdx.x / nchunk, fr0 = (blockIdx.x - b * nchunk) * CFG_RESCALE_ROWS;
    const float cs = cfg_sched_scale(scale, scale_row, t, t_row, sched, n_steps, m, b);
    const float phi = sched[(size_t)2 * n_steps + m];
    float f = 1.0f;
    if (cs != 1.0f && phi > 0.0f) {                                      // (block-uniform)
        const int len = lens ? min(max(lens[b], 0), frames) : frames;
        const double* pc = part + (size_t)b * frames * 4;
        double ak = 0.0, ae = 0.0;
        for (int r = tid; r < len; r += 128) { ak += pc[(size_t)r * 4]; ae += pc[(size_t)r * 4 + 2]; }
        block128_sum2(ak, ae, sh);
        const double mk = ak / (double)len, me = ae / (double)len, dw = (double)w;
        double qk = 0.0, qe = 0.0;
        for (int r = tid; r < len; r += 128) {
            const double dk = pc[(size_t)r * 4] - mk, de = pc[(size_t)r * 4 + 2] - me;
            qk += pc[(size_t)r * 4 + 1] + dw * (dk * dk);
            qe += pc[(size_t)r * 4 + 3] + dw * (de * de);
        }
        block128_sum2(qk, qe, sh);
        const double nn = (double)len * dw;
        if (nn >= 2.0) {                                                 // (every thread: the values are block-uniform)
            const double sdk = sqrt(qk / (nn - 1.0)), sde = sqrt(qe / (nn - 1.0));
            const double fd = (double)phi * sdk / sde + (1.0 - (double)phi);
            if (sde > 0.0 && sde <= 1.7976931348623157e308) f = (float)fd;
        }
    }
    const int total = min(CFG_RESCALE_ROWS, frames - fr0) * w;
    const float a1 = x0 ? c1[b] : 0.0f, a2 = x0 ? c2[b] : 0.0f;
    for (int i = tid; i < total; i += 128) {
        const int r = i / w, c = i - r * w;
        const size_t row = (size_t)b * frames + fr0 + r;
        float e = eps[row * lde + c0 + c];
        if (f != 1.0f) { e = rn_mul(f, e); eps[row * lde + c0 + c] = e; }
        if (x0) x0[row * ldx0 + c] = rn_sub(rn_mul(a1, x[row * ldx + c0 + c]), rn_mul(a2, e));
    }
}
int launch_cfg_mix_sched(const float* o, int ldo, int Mc, int cond_row0, int frames, int w, const float* scale, int scale_row,
                         const int64_t* t, int t_row, const float* sched, int n_steps, int m, bool rescale, const int* lens, double* part,
                         float* eps, int lde, int c0, const float* x, int ldx, const float* c1, const float* c2, float* x0, int ldx0,
                         hipStream_t s) {
    DSH_REQUIRE(scale && t && sched && n_steps > 0 && (m == 0 || m == 1), "cfg_mix_sched: needs the scales, the timesteps and the schedule table");
    DSH_REQUIRE(Mc > 0 && frames > 0 && Mc % frames == 0, "cfg_mix_sched: rows must be whole clips");
    DSH_REQUIRE(!rescale || part, "cfg_mix_sched: the rescale needs its row-moment scratch (4 fp64 per token row)");
    if (!rescale) {
        hipLaunchKernelGGL(cfg_mix_sched_kernel<false>, dim3(Mc), dim3(128), 0, s, o, ldo, cond_row0, frames, w, scale, scale_row, t, t_row, sched,
                           n_steps, m, lens, eps, lde, c0, x, ldx, c1, c2, x0, ldx0, nullptr);
        DSH_HIP_CHECK(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL(cfg_mix_sched_kernel<true>, dim3(Mc), dim3(128), 0, s, o, ldo, cond_row0, frames, w, scale, scale_row, t, t_row, sched,
                       n_steps, m, lens, eps, lde, c0, x, ldx, c1, c2, x0, ldx0, part);
    DSH_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(cfg_rescale_kernel, dim3((Mc / frames) * ceil_div(frames, CFG_RESCALE_ROWS)), dim3(128), 0, s, part, frames, w, scale, scale_row, t, t_row, sched, n_steps, m, lens, eps,
                       lde, c0, x, ldx, c1, c2, x0, ldx0);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Tiled activation layouts of the token-per-lane Linears (tl_linear.hip):
//   bf16: tile (tb, kt) = 32 tokens x 16 features (1 KB, 32 B per token);  fp32: per (tb, nt) four lane-native 1 KB pieces,
//   float index (((tb*NT + nt)*4 + qi)*64 + lane)*4 + e  <->  n = 32nt + 16(qi>>1) + 8h + 4(qi&1) + e, lane = (t&31) + 32h
typedef float tf32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t tile_pack2(float lo, float hi) { return pack_bf16_pair(lo, hi); }
__device__ __forceinline__ float tile_ld(const float* p) { return *p; }
__device__ __forceinline__ float tile_ld(const bf16* p) { return to_f32<bf16>(*p); }

typedef uint32_t tu32x4 __attribute__((ext_vector_type(4)));
__global__ void silu_f32_kernel(const float* x, float* y, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = silu_f(x[i]);
}
int launch_silu_f32(const float* x, float* y, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(silu_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, y, n);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

template <typename TS>
__global__ void tile_rows_bf16_kernel(const TS* src, int ld, int M, int w, char* dst, int Wd, size_t nchunk) {
    const int KT = Wd >> 4;
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < nchunk; c += (size_t)gridDim.x * blockDim.x) {
        const size_t tile = c >> 6;
        const int j = (int)(c & 63), m = j >> 1, hh = j & 1;
        const size_t tb = tile / KT;
        const int kt = (int)(tile % KT);
        const size_t t = tb * 32 + m;
        const int n0 = kt * 16 + hh * 8;
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (t < (size_t)M && n0 + i < w) ? tile_ld(src + t * ld + n0 + i) : 0.f;
        tu32x4 o;
        o.x = tile_pack2(v[0], v[1]); o.y = tile_pack2(v[2], v[3]); o.z = tile_pack2(v[4], v[5]); o.w = tile_pack2(v[6], v[7]);
        *reinterpret_cast<tu32x4*>(dst + c * 16) = o;
    }
}
template <typename TS>
int launch_tile_rows_bf16(const TS* src, int ld, int M, int w, void* dst, int Wd, hipStream_t s) {
    DSH_REQUIRE(Wd % 16 == 0 && w <= Wd && M > 0, "tile_rows: width must be a multiple of 16");
    const size_t nchunk = (size_t)ceil_div(M, 32) * (Wd >> 4) * 64;
    const int blocks = (int)std::min<size_t>((nchunk + 255) / 256, 16384);
    hipLaunchKernelGGL(tile_rows_bf16_kernel<TS>, dim3(blocks), dim3(256), 0, s, src, ld, M, w, reinterpret_cast<char*>(dst), Wd, nchunk);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}
template int launch_tile_rows_bf16<float>(const float*, int, int, int, void*, int, hipStream_t);
template int launch_tile_rows_bf16<bf16>(const bf16*, int, int, int, void*, int, hipStream_t);

// Given expression track of a gesture-only condition (denoiser.h, set_modality): src [M = B frames, E] fp32 -> what the expression encoder
// leaves behind for the gesture encoder's concat, in one launch: the fp32 rows x0 [M, ld] (columns E .. ld zero) and, on the bf16 path, the
// tiled bf16 operand x16 [round_up(M, 32), 128] with the rounding and layout of tile_rows_bf16_kernel (Wd = 128).  lens != null (ragged
// condition): frames >= lens[b] of clip b are written as zero whatever the caller's padding holds.
__global__ void pack_expr_track_kernel(const float* __restrict__ src, int E, int M, int frames, const int* __restrict__ lens, float* x0, int ld,
                                       char* x16, size_t nchunk) {
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < nchunk; c += (size_t)gridDim.x * blockDim.x) {
        const size_t tile = c >> 6;
        const int j = (int)(c & 63), m = j >> 1, hh = j & 1;
        const size_t tb = tile >> 3;
        const int kt = (int)(tile & 7);
        const size_t t = tb * 32 + m;
        const int n0 = kt * 16 + hh * 8;
        bool live = t < (size_t)M;
        if (live && lens) { const size_t b = t / (size_t)frames; live = (int)(t - b * frames) < lens[b]; }
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (live && n0 + i < E) ? src[t * E + n0 + i] : 0.f;
        if (t < (size_t)M) {
#pragma unroll
            for (int i = 0; i < 8; ++i) if (n0 + i < ld) x0[t * ld + n0 + i] = v[i];
        }
        if (x16) {
            tu32x4 o;
            o.x = tile_pack2(v[0], v[1]); o.y = tile_pack2(v[2], v[3]); o.z = tile_pack2(v[4], v[5]); o.w = tile_pack2(v[6], v[7]);
            *reinterpret_cast<tu32x4*>(x16 + c * 16) = o;
        }
    }
}
int launch_pack_expr_track(const float* src, int E, int B, int frames, const int* lens, float* x0, int ld, void* x16, hipStream_t s) {
    DSH_REQUIRE(src && x0 && B > 0 && frames > 0 && E > 0 && E <= ld && ld <= 128, "pack_expr_track: the expression width must fit the 128-column concat segment");
    const int M = B * frames;
    const size_t nchunk = (size_t)ceil_div(M, 32) * 8 * 64;
    const int blocks = (int)std::min<size_t>((nchunk + 255) / 256, 16384);
    hipLaunchKernelGGL(pack_expr_track_kernel, dim3(blocks), dim3(256), 0, s, src, E, M, frames, lens, x0, ld, reinterpret_cast<char*>(x16), nchunk);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// dst[r, c] for c in [c_lo, c_hi) of M rows of C columns <- src[r * src_ld + (c - c_lo)], or 0 when src is null: the inactive columns of a
// one-modality result (eps of dsh_eval, the final sample of dsh_sample)
__global__ void fill_cols_kernel(float* __restrict__ dst, int C, size_t M, int c_lo, int c_hi, const float* __restrict__ src, int src_ld) {
    const int w = c_hi - c_lo;
    const size_t n = M * (size_t)w, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const size_t r = i / (size_t)w;
        const int c = (int)(i - r * w);
        dst[r * C + c_lo + c] = src ? src[r * src_ld + c] : 0.f;
    }
}
int launch_fill_cols(float* dst, int C, size_t M, int c_lo, int c_hi, const float* src, int src_ld, hipStream_t s) {
    DSH_REQUIRE(dst && M > 0 && 0 <= c_lo && c_lo < c_hi && c_hi <= C && (!src || src_ld >= c_hi - c_lo), "fill_cols: invalid column window");
    const size_t n = M * (size_t)(c_hi - c_lo);
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(fill_cols_kernel, dim3(blocks), dim3(256), 0, s, dst, C, M, c_lo, c_hi, src, src_ld);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ void untile_rows_bf16_kernel(const char* src, int Wd, int M, int w, uint16_t* dst, int ld, size_t nchunk) {
    const int KT = Wd >> 4;
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < nchunk; c += (size_t)gridDim.x * blockDim.x) {
        const size_t tile = c >> 6;
        const int j = (int)(c & 63), m = j >> 1, hh = j & 1;
        const size_t tb = tile / KT;
        const int kt = (int)(tile % KT);
        const size_t t = tb * 32 + m;
        const int n0 = kt * 16 + hh * 8;
        if (t >= (size_t)M) continue;
        const tu32x4 v = *reinterpret_cast<const tu32x4*>(src + c * 16);
        const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (n0 + i < w) dst[t * ld + n0 + i] = (uint16_t)((i & 1) ? (wv[i >> 1] >> 16) : (wv[i >> 1] & 0xffffu));
    }
}
int launch_untile_rows_bf16(const void* src, int Wd, int M, int w, void* dst, int ld, hipStream_t s) {
    DSH_REQUIRE(Wd % 16 == 0 && w <= Wd && M > 0, "untile_rows: width must be a multiple of 16");
    const size_t nchunk = (size_t)ceil_div(M, 32) * (Wd >> 4) * 64;
    const int blocks = (int)std::min<size_t>((nchunk + 255) / 256, 16384);
    hipLaunchKernelGGL(untile_rows_bf16_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const char*>(src), Wd, M, w,
                       reinterpret_cast<uint16_t*>(dst), ld, nchunk);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

template <bool TO_TILED>
__global__ void tile_rows_f32_kernel(const float* src, float* dst, int ld, int M, int Wd, size_t npiece) {
    const int NT = Wd >> 5;
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < npiece; c += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(c & 63), qi = (int)((c >> 6) & 3);
        const size_t blk = c >> 8, tb = blk / NT;
        const int nt = (int)(blk % NT);
        const size_t t = tb * 32 + (lane & 31);
        const int n = 32 * nt + 16 * (qi >> 1) + 8 * (lane >> 5) + 4 * (qi & 1);
        if (TO_TILED) {
            tf32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (t < (size_t)M) v = *reinterpret_cast<const tf32x4*>(src + t * ld + n);
            *reinterpret_cast<tf32x4*>(dst + c * 4) = v;
        } else if (t < (size_t)M) {
            *reinterpret_cast<tf32x4*>(dst + t * ld + n) = *reinterpret_cast<const tf32x4*>(src + c * 4);
        }
    }
}
int launch_tile_rows_f32(const float* src, int ld, int M, float* dst, int Wd, hipStream_t s) {
    DSH_REQUIRE(Wd % 32 == 0 && ld % 4 == 0 && M > 0, "tile_rows_f32: width must be a multiple of 32");
    const size_t npiece = (size_t)ceil_div(M, 32) * (Wd >> 5) * 256;
    const int blocks = (int)std::min<size_t>((npiece + 255) / 256, 16384);
    hipLaunchKernelGGL(tile_rows_f32_kernel<true>, dim3(blocks), dim3(256), 0, s, src, dst, ld, M, Wd, npiece);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_untile_rows_f32(const float* src, int Wd, int M, float* dst, int ld, hipStream_t s) {
    DSH_REQUIRE(Wd % 32 == 0 && ld % 4 == 0 && M > 0, "untile_rows_f32: width must be a multiple of 32");
    const size_t npiece = (size_t)ceil_div(M, 32) * (Wd >> 5) * 256;
    const int blocks = (int)std::min<size_t>((npiece + 255) / 256, 16384);
    hipLaunchKernelGGL(tile_rows_f32_kernel<false>, dim3(blocks), dim3(256), 0, s, src, dst, ld, M, Wd, npiece);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// StylizationBlock coefficient fold (models/transformer.py:86-97): the stacked FiLM table rows [scale(D) | shift(D)] per
// block become [A | B] with A = gamma (1 + scale), B = beta (1 + scale) + shift, so that the token-per-lane prologue
// computes SiLU(((x - mean) rstd) A + B) with two coefficient vectors instead of four.  In place; gamma/beta: [nblk, D].
__global__ void film_fold_kernel(float* tab, int ld, int B, int nblk, int D, const float* gamma, const float* beta) {
    const size_t n = (size_t)B * nblk * D;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % D), j = (int)((i / D) % nblk);
        const size_t b = i / ((size_t)D * nblk);
        float* r = tab + b * ld + (size_t)j * 2 * D;
        const float sc = 1.0f + r[k], sh = r[D + k];
        r[k] = gamma[j * D + k] * sc;
        r[D + k] = fmaf(beta[j * D + k], sc, sh);
    }
}
int launch_film_fold(float* tab, int ld, int B, int nblk, int D, const float* gamma, const float* beta, hipStream_t s) {
    const size_t n = (size_t)B * nblk * D;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(film_fold_kernel, dim3(blocks), dim3(256), 0, s, tab, ld, B, nblk, D, gamma, beta);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// Round 6: FiLM rows are computed for the DISTINCT (timestep, speaker) rows only and expanded per clip here: dst[b] = fold(src[idx[b]])
// (idx == null: identity; fold == 0: plain copy — the fp32 path folds nothing).  One float4 per thread and piece.
__global__ void film_expand_kernel(const float* src, int ld, const int* idx, float* dst, int B, int nblk, int D, const float* gamma,
                                   const float* beta, int fold) {
    const int q4 = nblk * D / 4;                                 // float4 pieces per (row, half): [scale | shift] per block
    const size_t n = (size_t)B * q4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / q4;
        const int r = (int)(i % q4), j = r / (D / 4), k = (r % (D / 4)) * 4;
        const float* sr = src + (size_t)(idx ? idx[b] : (int)b) * ld + (size_t)j * 2 * D;
        float* dr = dst + b * ld + (size_t)j * 2 * D;
        tf32x4 sc = *reinterpret_cast<const tf32x4*>(sr + k), sh = *reinterpret_cast<const tf32x4*>(sr + D + k);
        if (fold) {
            const tf32x4 g = *reinterpret_cast<const tf32x4*>(gamma + j * D + k), be = *reinterpret_cast<const tf32x4*>(beta + j * D + k);
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float s1 = 1.0f + sc[e]; sh[e] = fmaf(be[e], s1, sh[e]); sc[e] = g[e] * s1; }
        }
        *reinterpret_cast<tf32x4*>(dr + k) = sc;
        *reinterpret_cast<tf32x4*>(dr + D + k) = sh;
    }
}
int launch_film_expand(const float* src, int ld, const int* idx, float* dst, int B, int nblk, int D, const float* gamma, const float* beta,
                       int fold, hipStream_t s) {
    DSH_REQUIRE(D % 4 == 0 && ld % 4 == 0, "film_expand: widths must be multiples of 4");
    const size_t n = (size_t)B * (nblk * D / 4);
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(film_expand_kernel, dim3(blocks), dim3(256), 0, s, src, ld, idx, dst, B, nblk, D, gamma, beta, fold);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}
// dst[b, :w] = src[idx[b], :w]  (fp32 rows; the speaker embedding per clip from the distinct speakers' rows)
__global__ void gather_rows_f32_kernel(const float* src, int ld, const int* idx, float* dst, int ldd, int B, int w) {
    const size_t n = (size_t)B * w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / w; const int k = (int)(i % w);
        dst[b * ldd + k] = src[(size_t)idx[b] * ld + k];
    }
}
int launch_gather_rows_f32(const float* src, int ld, const int* idx, float* dst, int ldd, int B, int w, hipStream_t s) {
    const size_t n = (size_t)B * w;
    hipLaunchKernelGGL(gather_rows_f32_kernel, dim3((int)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, s, src, ld, idx, dst, ldd, B, w);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// one thread = 8 consecutive features of one token: two fp32 pieces (qi = 2c, 2c+1) + one 16-byte bf16 chunk, per CFG half
__global__ void seed_stream_kernel(const float* h0, int Mc, int D, const float* cadd, int has_null, int row1, float* h,
                                   char* h16, char* hlo, size_t nitem) {
    const int NT = D >> 5;
    for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < nitem; it += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(it & 63), c = (int)((it >> 6) & 1);
        const size_t blk = it >> 7, tb = blk / NT;
        const int nt = (int)(blk % NT);
        const size_t t = tb * 32 + (lane & 31);
        if (t >= (size_t)Mc) continue;
        const int hh = lane >> 5, n = 32 * nt + 16 * c + 8 * hh;
        const tf32x4 a = *reinterpret_cast<const tf32x4*>(h0 + t * D + n), b = *reinterpret_cast<const tf32x4*>(h0 + t * D + n + 4);
        const int lane_off = (lane & 31) * 32 + hh * 16;
        for (int half = 0; half < 1 + has_null; ++half) {
            tf32x4 va = a, vb = b;
            if (half == 0 && has_null) {
                va += *reinterpret_cast<const tf32x4*>(cadd + n);
                vb += *reinterpret_cast<const tf32x4*>(cadd + n + 4);
            }
            const size_t tbh = tb + (half ? (size_t)(row1 >> 5) : 0);
            tu32x4 o;
            o.x = tile_pack2(va.x, va.y); o.y = tile_pack2(va.z, va.w); o.z = tile_pack2(vb.x, vb.y); o.w = tile_pack2(vb.z, vb.w);
            *reinterpret_cast<tu32x4*>(h16 + (tbh * (2 * NT) + 2 * nt + c) * 1024 + lane_off) = o;
            if (hlo) {       // residual stream as (hi, lo) bf16 planes: lo = bf16(h - hi)
                const float v[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
                const uint32_t hw[4] = {o.x, o.y, o.z, o.w};
                tu32x4 l;
                uint32_t lw[4];
                for (int j = 0; j < 4; ++j)
                    lw[j] = tile_pack2(v[2 * j] - __builtin_bit_cast(float, hw[j] << 16), v[2 * j + 1] - __builtin_bit_cast(float, hw[j] & 0xffff0000u));
                l.x = lw[0]; l.y = lw[1]; l.z = lw[2]; l.w = lw[3];
                *reinterpret_cast<tu32x4*>(hlo + (tbh * (2 * NT) + 2 * nt + c) * 1024 + lane_off) = l;
            } else {
                float* hp = h + (((tbh * NT + nt) * 4 + 2 * c) * 64 + lane) * 4;
                *reinterpret_cast<tf32x4*>(hp) = va;
                *reinterpret_cast<tf32x4*>(hp + 256) = vb;
            }
        }
    }
}
int launch_seed_stream(const float* h0, int Mc, int D, const float* c, int has_null, int row1, float* h, void* h16, hipStream_t s, void* hlo) {
    DSH_REQUIRE(D % 32 == 0 && (!has_null || (row1 % 32 == 0 && row1 >= Mc && c)), "seed_stream: bad arguments");
    const size_t nitem = (size_t)ceil_div(Mc, 32) * (D >> 5) * 128;
    const int blocks = (int)std::min<size_t>((nitem + 255) / 256, 16384);
    hipLaunchKernelGGL(seed_stream_kernel, dim3(blocks), dim3(256), 0, s, h0, Mc, D, c, has_null, row1, h, reinterpret_cast<char*>(h16),
                       reinterpret_cast<char*>(hlo), nitem);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// row-major fp32 <-> (hi, lo) bf16 planes, tiled (one thread = 8 consecutive features of one token = one 16-byte chunk per plane)
template <bool TO_PLANES>
__global__ void hilo_rows_kernel(float* rm, int ld, int M, int w, char* hi, char* lo, int Wd, size_t nchunk) {
    const int KT = Wd >> 4;
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < nchunk; c += (size_t)gridDim.x * blockDim.x) {
        const size_t tile = c >> 6;
        const int j = (int)(c & 63), m = j >> 1, hh = j & 1;
        const size_t tb = tile / KT;
        const int kt = (int)(tile % KT);
        const size_t t = tb * 32 + m;
        const int n0 = kt * 16 + hh * 8;
        if (TO_PLANES) {
            float v[8];
            for (int i = 0; i < 8; ++i) v[i] = (t < (size_t)M && n0 + i < w) ? rm[t * ld + n0 + i] : 0.f;
            uint32_t hw[4], lw[4];
            for (int i = 0; i < 4; ++i) {
                hw[i] = tile_pack2(v[2 * i], v[2 * i + 1]);
                lw[i] = tile_pack2(v[2 * i] - __builtin_bit_cast(float, hw[i] << 16), v[2 * i + 1] - __builtin_bit_cast(float, hw[i] & 0xffff0000u));
            }
            tu32x4 a, b;
            a.x = hw[0]; a.y = hw[1]; a.z = hw[2]; a.w = hw[3]; b.x = lw[0]; b.y = lw[1]; b.z = lw[2]; b.w = lw[3];
            *reinterpret_cast<tu32x4*>(hi + c * 16) = a;
            *reinterpret_cast<tu32x4*>(lo + c * 16) = b;
        } else if (t < (size_t)M) {
            const tu32x4 a = *reinterpret_cast<const tu32x4*>(hi + c * 16), b = *reinterpret_cast<const tu32x4*>(lo + c * 16);
            const uint32_t hw[4] = {a.x, a.y, a.z, a.w}, lw[4] = {b.x, b.y, b.z, b.w};
            for (int i = 0; i < 8; ++i) {
                if (n0 + i >= w) continue;
                const uint32_t h2 = hw[i >> 1], l2 = lw[i >> 1];
                const float fh = __builtin_bit_cast(float, (i & 1) ? (h2 & 0xffff0000u) : (h2 << 16));
                const float fl = __builtin_bit_cast(float, (i & 1) ? (l2 & 0xffff0000u) : (l2 << 16));
                rm[t * ld + n0 + i] = fh + fl;
            }
        }
    }
}
int launch_tile_rows_hilo(const float* src, int ld, int M, int w, void* hi, void* lo, int Wd, hipStream_t s) {
    DSH_REQUIRE(Wd % 16 == 0 && w <= Wd && M > 0, "tile_rows_hilo: width must be a multiple of 16");
    const size_t nchunk = (size_t)ceil_div(M, 32) * (Wd >> 4) * 64;
    const int blocks = (int)std::min<size_t>((nchunk + 255) / 256, 16384);
    hipLaunchKernelGGL(hilo_rows_kernel<true>, dim3(blocks), dim3(256), 0, s, const_cast<float*>(src), ld, M, w, reinterpret_cast<char*>(hi),
                       reinterpret_cast<char*>(lo), Wd, nchunk);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_untile_rows_hilo(const void* hi, const void* lo, int Wd, int M, int w, float* dst, int ld, hipStream_t s) {
    DSH_REQUIRE(Wd % 16 == 0 && w <= Wd && M > 0, "untile_rows_hilo: width must be a multiple of 16");
    const size_t nchunk = (size_t)ceil_div(M, 32) * (Wd >> 4) * 64;
    const int blocks = (int)std::min<size_t>((nchunk + 255) / 256, 16384);
    hipLaunchKernelGGL(hilo_rows_kernel<false>, dim3(blocks), dim3(256), 0, s, dst, ld, M, w, reinterpret_cast<char*>(const_cast<void*>(hi)),
                       reinterpret_cast<char*>(const_cast<void*>(lo)), Wd, nchunk);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace dsh

// ------------------------------------------------------------------------------------------------
// Rows either side of the sampling path (SURVEY.md §8f "next"):
//   interp_time   F.interpolate(x^T, size=T, mode='linear', align_corners=True)^T along frames
//                 (datasets/show.py:98, trainers/ddpm_show_trainer.py:1082: HuBERT features -> pose frame rate)
//   affine_cols   inv_standardize: y = x * std[c] + mean[c]          (datasets/show.py:157-162)
namespace dsh {

// output frame t of Tout from the Tin frames at xb
__device__ __forceinline__ void interp_time_row(const float* xb, int Tin, int C, float* yr, int t, int Tout) {
    // align_corners=True: src = t * (Tin - 1) / (Tout - 1); Tout == 1 samples frame 0 (ATen area_pixel_compute_scale)
    const float scale = Tout > 1 ? (float)(Tin - 1) / (float)(Tout - 1) : 0.0f;
    const float src = scale * (float)t;
    int i0 = (int)src;
    if (i0 > Tin - 1) i0 = Tin - 1;
    const int i1 = i0 + (i0 < Tin - 1 ? 1 : 0);
    const float w1 = src - (float)i0, w0 = 1.0f - w1;
    const float* x0 = xb + (size_t)i0 * C;
    const float* x1 = xb + (size_t)i1 * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) yr[c] = w0 * x0[c] + w1 * x1[c];
}

__global__ void interp_time_kernel(const float* x, int B, int Tin, int C, float* y, int Tout) {
    const int row = blockIdx.x;                 // b * Tout + t
    const int b = row / Tout, t = row % Tout;
    interp_time_row(x + (size_t)b * Tin * C, Tin, C, y + (size_t)row * C, t, Tout);
}

// x [B, Tin, C] -> y [B, Tout, C] with a frame count of its own per row on both sides (clamped to the padded sizes): row b is the dense kernel on
// (lens_in[b], lens_out[b]); frames t >= lens_out[b] are 0, and so is a row without input frames.  No frame >= lens_in[b] is read.
__global__ void interp_time_ragged_kernel(const float* x, int B, int Tin, int C, float* y, int Tout, const int* __restrict__ lens_in,
                                          const int* __restrict__ lens_out) {
    const int row = blockIdx.x;
    const int b = row / Tout, t = row % Tout;
    const int tin = min(lens_in[b], Tin), tout = min(lens_out[b], Tout);
    float* yr = y + (size_t)row * C;
    if (t >= tout || tin < 1) {
        for (int c = threadIdx.x; c < C; c += blockDim.x) yr[c] = 0.0f;
        return;
    }
    interp_time_row(x + (size_t)b * Tin * C, tin, C, yr, t, tout);
}

int launch_interp_time(const float* x, int B, int Tin, int C, float* y, int Tout, hipStream_t s) {
    DSH_REQUIRE(B > 0 && Tin > 0 && Tout > 0 && C > 0, "interp_time: dims must be positive");
    hipLaunchKernelGGL(interp_time_kernel, dim3(B * Tout), dim3(256), 0, s, x, B, Tin, C, y, Tout);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_interp_time_ragged(const float* x, int B, int Tin, int C, float* y, int Tout, const int* lens_in, const int* lens_out, hipStream_t s) {
    DSH_REQUIRE(x && y && lens_in && lens_out, "interp_time (ragged): null pointer");
    DSH_REQUIRE(B > 0 && Tin > 0 && Tout > 0 && C > 0 && (long long)B * Tout < (1ll << 31), "interp_time (ragged): dims must be positive");
    hipLaunchKernelGGL(interp_time_ragged_kernel, dim3(B * Tout), dim3(256), 0, s, x, B, Tin, C, y, Tout, lens_in, lens_out);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ void affine_cols_kernel(const float* x, size_t n, int C, const float* mean, const float* stdv, float* y) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % (size_t)C);
        y[i] = rn_add(rn_mul(x[i], stdv[c]), mean[c]);
    }
}

int launch_affine_cols(const float* x, size_t n, int C, const float* mean, const float* stdv, float* y, hipStream_t s) {
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(affine_cols_kernel, dim3((unsigned)(blocks < 2048 ? (blocks ? blocks : 1) : 2048)), dim3(256), 0, s, x, n, C,
                       mean, stdv, y);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace dsh
