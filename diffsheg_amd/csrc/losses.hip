// Denoising loss terms on the device: the eval-mode forward of the reference's training objective (GaussianDiffusion.training_losses,
// models/gaussian_diffusion.py:1319-1426, epsilon / MSE branch; the arithmetic of backward_G, trainers/ddpm_beat_trainer.py:222-260) from
// eps, noise, x_t and x0 [B, T, C] fp32.  Two launches on the caller's stream, no synchronisation, no floating-point atomics: block partials
// in a scratch area behind the results, summed in a fixed order — two runs give identical bits.
//
//  (1) loss_partials: one block per (row b, chunk of LOSS_FRAMES frames).  The block copies its frames of the four tensors plus ONE halo
//      frame (the velocity term's neighbour f + 1, when the row owns it) into LDS — every element is read from HBM once, the halo frame
//      twice — and computes from LDS in chunk-relative element order.  The copy is the only part that looks at addresses: whole 16-byte
//      vectors where the tile's byte range allows (neither C nor the split is a multiple of 4, so a row, a chunk and both sides of the
//      split start at any 4-byte offset: a scalar head up to the first 16-byte boundary, float4 body, scalar tail, per tensor), scalar
//      loads for tiles too small to be worth it.  Each tensor's tile sits in LDS at the same offset mod 16 bytes as in HBM, so the body is
//      ds_write_b128.  Both copies leave the same LDS image; the arithmetic never sees which one ran, nor where the row lies in the batch.
//        x0_pred = c1 x_t - c2 eps      rn_mul / rn_sub, individually rounded: the bits dsh_op_ddim_step_full writes to x0_out
//        d_n = eps - noise;  d_0 = x0_pred - x0;  d_v = (x0_pred[f] - x0_pred[f+1]) - (x0[f] - x0[f+1]);  z = |x0 / beta - x0_pred / beta|
//      every difference and quotient one rounded fp32 operation, as torch computes them; squares, the Huber value (z < 1: z^2 / 2, else
//      z - 1 / 2) and all sums in fp64.  Thread-local sums in element order, a shuffle tree per wave, the four waves in order.
//      Frames >= lens[b] are never read (NaN there changes nothing); their x0_pred / frame_mse outputs are written as 0.
//  (2) loss_finalize: per row the chunk partials in ascending chunk order (a row's numbers depend on nothing but the row: an empty chunk
//      adds +0), the counts, then the batch scalars.
#include "../../include/diffsheg_hip.h"
#include "losses.h"

namespace dsh {

constexpr int LOSS_FRAMES = 8, LOSS_THREADS = 256, LOSS_SUMS = 5;
constexpr int LOSS_MAX_C = 448;              // 4 tensors x 9 frames x C floats (+ 3 floats of alignment slack each) within 64 KB of LDS
constexpr int LOSS_VEC_MIN = 1024;           // floats per tile from which the copy uses 16-byte vectors
constexpr int LOSS_RED_BYTES = 4 * 8 * 2;    // reduction scratch in front of the tiles: keeps the tiles 16-byte aligned

// fixed-order block reduction (shuffle tree inside a wave, then the 4 waves in order)
__device__ __forceinline__ double loss_block_sum(double v, double* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    double r = sm[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r += sm[w];
    __syncthreads();
    return r;
}

// n floats from g (4-byte aligned) into the LDS region `region` (16-byte aligned, n + 3 floats): returns the tile's base, which has the
// alignment mod 16 bytes of g
template <bool VEC>
__device__ __forceinline__ const float* loss_stage(float* region, const float* __restrict__ g, int n) {
    const int tid = threadIdx.x;
    const int mis = (int)(((uintptr_t)g >> 2) & 3u);
    float* s = region + mis;
    if (!VEC) {
        for (int i = tid; i < n; i += LOSS_THREADS) s[i] = g[i];
        return s;
    }
    const int head = min(n, (4 - mis) & 3);
    const int nv = (n - head) >> 2;
    if (tid < head) s[tid] = g[tid];
    const float4* gv = reinterpret_cast<const float4*>(g + head);
    float4* sv = reinterpret_cast<float4*>(s + head);
    for (int v = tid; v < nv; v += LOSS_THREADS) sv[v] = gv[v];
    for (int i = head + 4 * nv + tid; i < n; i += LOSS_THREADS) s[i] = g[i];
    return s;
}

template <bool VEC>
__global__ __launch_bounds__(LOSS_THREADS) void loss_partials(const float* __restrict__ eps, const float* __restrict__ noise,
                                                              const float* __restrict__ x_t, const float* __restrict__ x0,
                                                              const float* __restrict__ c1v, const float* __restrict__ c2v,
                                                              const int* __restrict__ lens, int T, int C, int split, float beta, int n_chunks,
                                                              int region_floats, float* __restrict__ x0_out, float* __restrict__ frame_mse,
                                                              double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char loss_smem[];
    double* red = reinterpret_cast<double*>(loss_smem);
    float* tiles = reinterpret_cast<float*>(loss_smem + LOSS_RED_BYTES);
    const int tid = threadIdx.x;
    const int b = blockIdx.x / n_chunks, k = blockIdx.x - b * n_chunks;
    const int f0 = k * LOSS_FRAMES;
    const int len = lens ? min(max(lens[b], 0), T) : T;
    const int nf = min(LOSS_FRAMES, len - f0);                  // frames of this chunk the row owns (<= 0: none)
    const int nf_pad = min(LOSS_FRAMES, T - f0);                // frames of this chunk inside the padded row
    const size_t base = ((size_t)b * T + f0) * C;
    double* my_part = part + (size_t)blockIdx.x * LOSS_SUMS;
    if (nf <= 0) {                                              // (the whole block takes this branch)
        if (tid < LOSS_SUMS) my_part[tid] = 0.0;
        if (x0_out)
            for (int i = tid; i < nf_pad * C; i += LOSS_THREADS) x0_out[base + i] = 0.0f;
        if (frame_mse && tid < nf_pad) frame_mse[(size_t)b * T + f0 + tid] = 0.0f;
        return;
    }
    const int halo = (f0 + nf < len) ? 1 : 0;
    const int n_own = nf * C, n_all = (nf + halo) * C;
    const float* s_eps = loss_stage<VEC>(tiles, eps + base, n_all);
    const float* s_nz = loss_stage<VEC>(tiles + region_floats, noise + base, n_own);
    const float* s_xt = loss_stage<VEC>(tiles + 2 * region_floats, x_t + base, n_all);
    const float* s_x0 = loss_stage<VEC>(tiles + 3 * region_floats, x0 + base, n_all);
    __syncthreads();
    const float c1 = c1v[b], c2 = c2v[b];
    const int n_pair = (nf - 1 + halo) * C;                     // elements whose frame f + 1 belongs to the row
    double a_ges = 0.0, a_exp = 0.0, a_x0 = 0.0, a_vel = 0.0, a_hub = 0.0;
    for (int i = tid; i < n_own; i += LOSS_THREADS) {
        const int c = i % C;
        const float e = s_eps[i], x0v = s_x0[i];
        const float dn = rn_sub(e, s_nz[i]);
        const double sq = (double)dn * (double)dn;
        if (c < split) a_ges += sq; else a_exp += sq;
        const float xp = rn_sub(rn_mul(c1, s_xt[i]), rn_mul(c2, e));
        if (x0_out) x0_out[base + i] = xp;
        const float d0 = rn_sub(xp, x0v);
        a_x0 += (double)d0 * (double)d0;
        if (i < n_pair) {
            const int j = i + C;
            const float xp_n = rn_sub(rn_mul(c1, s_xt[j]), rn_mul(c2, s_eps[j]));
            const float dv = rn_sub(rn_sub(xp, xp_n), rn_sub(x0v, s_x0[j]));
            a_vel += (double)dv * (double)dv;
        }
        const double z = (double)fabsf(rn_sub(__fdiv_rn(x0v, beta), __fdiv_rn(xp, beta)));
        a_hub += z < 1.0 ? 0.5 * z * z : z - 0.5;
    }
    if (x0_out)
        for (int i = n_own + tid; i < nf_pad * C; i += LOSS_THREADS) x0_out[base + i] = 0.0f;
    if (frame_mse) {
        // one wave per frame: mean over C of (eps - noise)^2, lanes strided over the columns, a fixed shuffle tree
        const int lane = tid & 63;
        for (int f = tid >> 6; f < nf_pad; f += LOSS_THREADS / 64) {
            double m = 0.0;
            if (f < nf)
                for (int c = lane; c < C; c += 64) {
                    const float dn = rn_sub(s_eps[f * C + c], s_nz[f * C + c]);
                    m += (double)dn * (double)dn;
                }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
            if (lane == 0) frame_mse[(size_t)b * T + f0 + f] = (float)(m / (double)C);
        }
    }
    const double r0 = loss_block_sum(a_ges, red), r1 = loss_block_sum(a_exp, red), r2 = loss_block_sum(a_x0, red);
    const double r3 = loss_block_sum(a_vel, red), r4 = loss_block_sum(a_hub, red);
    if (tid == 0) { my_part[0] = r0; my_part[1] = r1; my_part[2] = r2; my_part[3] = r3; my_part[4] = r4; }
}

// one block: the rows strided over the threads (each row's chunks in ascending order), then a fixed-order block sum for the batch
__global__ __launch_bounds__(LOSS_THREADS) void loss_finalize(const double* __restrict__ part, const int* __restrict__ lens, int B, int T, int C,
                                                              int n_chunks, double beta, double* __restrict__ res) {
    __shared__ double red[4];
    double t_eps = 0.0, t_vel = 0.0, t_hub = 0.0, t_frames = 0.0, t_pairs = 0.0;
    double* rows = res + DSH_LOSS_HEADER;
    for (int b = threadIdx.x; b < B; b += LOSS_THREADS) {
        const int len = lens ? min(max(lens[b], 0), T) : T;
        double s[LOSS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < n_chunks; ++k)
#pragma unroll
            for (int j = 0; j < LOSS_SUMS; ++j) s[j] += part[((size_t)b * n_chunks + k) * LOSS_SUMS + j];
        double* r = rows + (size_t)b * DSH_LOSS_COLS;
#pragma unroll
        for (int j = 0; j < LOSS_SUMS; ++j) r[j] = s[j];
        r[5] = (double)len * (double)C;
        r[6] = (double)max(len - 1, 0);
        t_eps += s[0] + s[1]; t_vel += s[3]; t_hub += s[4]; t_frames += (double)len; t_pairs += (double)max(len - 1, 0);
    }
    t_eps = loss_block_sum(t_eps, red); t_vel = loss_block_sum(t_vel, red); t_hub = loss_block_sum(t_hub, red);
    t_frames = loss_block_sum(t_frames, red); t_pairs = loss_block_sum(t_pairs, red);
    if (threadIdx.x == 0) {
        // backward_G, trainers/ddpm_beat_trainer.py:222-260 (ddpm_show_trainer.py:199-237 is the same code), mirrored literally:
        //  * :231 recomputes loss_model_pred over all channels and overwrites the expr_weight form of :223-230, so expr_weight has no
        //    effect; the gesture and expression sums are kept apart in the row terms, and added here;
        //  * :245 scales the velocity term by 100 for the log, but :247 adds the UNSCALED loss_vel_rec (the local, not self.loss_vel_rec)
        //    to final_loss; :255-257 add the scaled Huber term.
        // masked means: src_mask is 1 on a row's own frames; the Huber mean is over the valid elements.  A zero count gives 0, not NaN
        // (the counts are in the header; the Python callers refuse a batch without a pair).
        const double dC = (double)C;
        const double model_pred = t_frames > 0.0 ? t_eps / dC / t_frames : 0.0;
        const double vel = t_pairs > 0.0 ? t_vel / dC / t_pairs : 0.0;
        const double hub = t_frames > 0.0 ? t_hub / (t_frames * dC) * beta : 0.0;
        res[0] = 1000.0 * model_pred;
        res[1] = 100.0 * vel;
        res[2] = 100.0 * hub;
        res[3] = res[0] + vel + res[2];
        res[4] = t_frames;
        res[5] = t_pairs;
        res[6] = t_frames * dC;
        res[7] = 0.0;
    }
}

static int loss_chunks(int T) { return (T + LOSS_FRAMES - 1) / LOSS_FRAMES; }

long long denoise_losses_result_bytes(int B, int T) {
    if (B <= 0 || T <= 0) return -1;
    return ((long long)DSH_LOSS_HEADER + (long long)B * DSH_LOSS_COLS + (long long)B * loss_chunks(T) * LOSS_SUMS) * 8;
}

int launch_denoise_losses(const float* eps, const float* noise, const float* x_t, const float* x0, const float* c1_dev, const float* c2_dev,
                          const int* lens_dev, int B, int T, int C, int split, float huber_beta, float* x0_pred_out, float* frame_mse_out,
                          void* result_dev, hipStream_t s) {
    DSH_REQUIRE(eps && noise && x_t && x0 && c1_dev && c2_dev && result_dev, "dsh_op_denoise_losses: null pointer");
    DSH_REQUIRE(B > 0 && T > 0 && C > 0, "dsh_op_denoise_losses: dims must be positive");
    DSH_REQUIRE(C <= LOSS_MAX_C, "dsh_op_denoise_losses: at most 448 channels (nine frames of the four tensors are staged in 64 KB of LDS)");
    DSH_REQUIRE(split > 0 && split < C, "dsh_op_denoise_losses: split must lie inside (0, C)");
    DSH_REQUIRE(huber_beta > 0.0f, "dsh_op_denoise_losses: huber_beta must be positive");
    const int n_chunks = loss_chunks(T);
    DSH_REQUIRE((long long)B * n_chunks < (1LL << 31), "dsh_op_denoise_losses: too many blocks (B * ceil(T / 8) must stay below 2^31)");
    const uintptr_t a4 = (uintptr_t)eps | (uintptr_t)noise | (uintptr_t)x_t | (uintptr_t)x0 | (uintptr_t)c1_dev | (uintptr_t)c2_dev |
                         (uintptr_t)lens_dev | (uintptr_t)x0_pred_out | (uintptr_t)frame_mse_out;
    DSH_REQUIRE(a4 % 4 == 0, "dsh_op_denoise_losses: tensors must be 4-byte aligned");
    DSH_REQUIRE(((uintptr_t)result_dev % 8) == 0, "dsh_op_denoise_losses: result buffer must be 8-byte aligned");
    double* res = reinterpret_cast<double*>(result_dev);
    double* part = res + DSH_LOSS_HEADER + (size_t)B * DSH_LOSS_COLS;
    const int tile = (LOSS_FRAMES + 1) * C;
    const int region_floats = (tile + 3 + 3) / 4 * 4;          // + 3 floats of alignment slack, rounded up to whole 16-byte vectors
    const size_t lds = LOSS_RED_BYTES + (size_t)4 * region_floats * sizeof(float);
    const dim3 grid((unsigned)((long long)B * n_chunks)), block(LOSS_THREADS);
    if (tile >= LOSS_VEC_MIN)
        hipLaunchKernelGGL(loss_partials<true>, grid, block, lds, s, eps, noise, x_t, x0, c1_dev, c2_dev, lens_dev, T, C, split, huber_beta,
                           n_chunks, region_floats, x0_pred_out, frame_mse_out, part);
    else
        hipLaunchKernelGGL(loss_partials<false>, grid, block, lds, s, eps, noise, x_t, x0, c1_dev, c2_dev, lens_dev, T, C, split, huber_beta,
                           n_chunks, region_floats, x0_pred_out, frame_mse_out, part);
    DSH_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(loss_finalize, dim3(1), dim3(LOSS_THREADS), 0, s, part, lens_dev, B, T, C, n_chunks, (double)huber_beta, res);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace dsh
