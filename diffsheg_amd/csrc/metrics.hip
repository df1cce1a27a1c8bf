// Per-batch validation metrics on the device (trainers/ddpm_show_trainer.py:516-550, ddpm_beat_trainer.py:587-597): MSE, PCK and the
// pairwise-L1 diversity of `outputs` against `motions`, [B, T, C] fp32.  Three launches on the caller's stream, no synchronisation, no
// floating-point atomics: block partials in a scratch area behind the results, summed in a fixed order by the last launch — two runs give
// identical bits.
//
//  (1) mse_pck_partials: one pass over both tensors.  diff = o - m; sum diff^2 accumulated in fp64 per thread; PCK counts the joints
//      (joint_dim = 1: every element, SHOW; 3: consecutive triplets, BEAT) with sqrt(sum_j diff_j^2) < 0.5 computed as the reference does
//      in fp32: individually rounded products and sums ((d0 d0 + d1 d1) + d2 d2, contraction off: hipcc would otherwise fuse a*a + b
//      into an FMA) and a correctly rounded square root (fp64 sqrt of the fp32 sum rounded back to fp32: 53 >= 2 * 24 + 2 bits, so the
//      double rounding is innocuous), so that the count can be compared exactly.
//  (2) diversity_partials: for each complete group of b_div consecutive clips, sum_{i<j} sum_e |o_i[e] - o_j[e]|.  A block owns 256
//      element columns of one group: it stages the b_div x 256 values in LDS once (each element of `outputs` is read from HBM exactly
//      once, coalesced) and every thread walks all pairs of its own column — LDS reads are conflict-free (consecutive lanes,
//      consecutive banks) and there are b_div (b_div - 1) / 2 of them per element.  Inner sums over j in fp32 (< b_div terms), the rest
//      in fp64.
//  (3) metrics_finalize: fixed-order sums of the partials, the means and the per-group diversity values.
#include "../../include/diffsheg_hip.h"
#include "fgd.h"

namespace dsh {

constexpr int MP_BLOCKS = 1024, MP_THREADS = 256;
constexpr int DV_COLS = 256;
constexpr int DV_MAX_BDIV = 128;             // b_div x 256 floats of LDS: 128 KB at the limit (the reference uses min(50, B))

// fixed-order block reduction (shuffle tree inside a wave, then the 4 waves in order)
template <typename V>
__device__ __forceinline__ V block_sum_256(V v, V* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    V r = sm[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r += sm[w];
    __syncthreads();
    return r;
}

__device__ __forceinline__ bool pck_hit(float s) { return (float)sqrt((double)s) < 0.5f; }

__global__ __launch_bounds__(MP_THREADS) void mse_pck_partials(const float* __restrict__ o, const float* __restrict__ m, long long n_joints,
                                                               int joint_dim, double* __restrict__ part_sum, long long* __restrict__ part_cnt) {
#pragma clang fp contract(off)
    __shared__ double sm_d[4];
    __shared__ long long sm_c[4];
    double sum = 0.0;
    long long cnt = 0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n_joints; j += stride) {
        if (joint_dim == 1) {
            const float d = o[j] - m[j];
            const float s = d * d;
            sum += (double)d * (double)d;
            cnt += pck_hit(s) ? 1 : 0;
        } else {
            const long long e = 3 * j;
            const float d0 = o[e] - m[e], d1 = o[e + 1] - m[e + 1], d2 = o[e + 2] - m[e + 2];
            const float p0 = d0 * d0, p1 = d1 * d1, p2 = d2 * d2;
            const float s01 = p0 + p1;
            const float s = s01 + p2;
            sum += ((double)d0 * (double)d0 + (double)d1 * (double)d1) + (double)d2 * (double)d2;
            cnt += pck_hit(s) ? 1 : 0;
        }
    }
    const double bs = block_sum_256<double>(sum, sm_d);
    const long long bc = block_sum_256<long long>(cnt, sm_c);
    if (threadIdx.x == 0) { part_sum[blockIdx.x] = bs; part_cnt[blockIdx.x] = bc; }
}

__global__ __launch_bounds__(DV_COLS) void diversity_partials(const float* __restrict__ o, long long clip_elems, int b_div, int n_chunks,
                                                              double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float sv[];     // [b_div][DV_COLS]
    __shared__ double sm_d[4];
    const int g = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const long long e = (long long)chunk * DV_COLS + tid;
    const bool ok = e < clip_elems;
    const float* base = o + (size_t)g * b_div * clip_elems;
    for (int i = 0; i < b_div; ++i) sv[i * DV_COLS + tid] = ok ? base[(size_t)i * clip_elems + e] : 0.0f;
    // (every thread reads back only its own column: no barrier needed before the pair loop)
    double tot = 0.0;
    for (int i = 0; i + 1 < b_div; ++i) {
        const float vi = sv[i * DV_COLS + tid];
        float s = 0.0f;
        for (int j = i + 1; j < b_div; ++j) s += fabsf(vi - sv[j * DV_COLS + tid]);
        tot += (double)s;
    }
    const double bs = block_sum_256<double>(tot, sm_d);
    if (tid == 0) part[(size_t)g * n_chunks + chunk] = bs;
}

// one wave: lanes take the partials strided, then a fixed shuffle tree
__global__ __launch_bounds__(64) void metrics_finalize(const double* __restrict__ part_sum, const long long* __restrict__ part_cnt,
                                                       const double* __restrict__ part_div, int n_chunks, int groups, int b_div,
                                                       long long n_elems, long long n_joints, long long clip_elems, double* __restrict__ res) {
    const int lane = threadIdx.x;
    double s = 0.0;
    long long c = 0;
    for (int i = lane; i < MP_BLOCKS; i += 64) { s += part_sum[i]; c += part_cnt[i]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); c += __shfl_xor(c, o, 64); }
    long long* res_i = reinterpret_cast<long long*>(res);
    if (lane == 0) {
        res[0] = s;
        res_i[1] = c;
        res[2] = s / (double)n_elems;
        res[3] = (double)c / (double)n_joints;
        res_i[4] = groups;
    }
    for (int g = 0; g < groups; ++g) {
        double d = 0.0;
        for (int i = lane; i < n_chunks; i += 64) d += part_div[(size_t)g * n_chunks + i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
        if (lane == 0) res[DSH_METRICS_HEADER + g] = d / (double)clip_elems * 2.0 / ((double)b_div * (double)(b_div - 1));
    }
}

long long batch_metrics_result_bytes(int B, int T, int C, int b_div) {
    if (B <= 0 || T <= 0 || C <= 0 || b_div < 1) return -1;
    const long long clip_elems = (long long)T * C, groups = B / b_div, n_chunks = (clip_elems + DV_COLS - 1) / DV_COLS;
    return (DSH_METRICS_HEADER + groups + 2 * MP_BLOCKS + groups * n_chunks) * 8;
}

int launch_batch_metrics(const float* outputs, const float* motions, int B, int T, int C, int joint_dim, int b_div, void* result_dev,
                         hipStream_t s) {
    DSH_REQUIRE(outputs && motions && result_dev, "dsh_op_batch_metrics: null pointer");
    DSH_REQUIRE(B > 0 && T > 0 && C > 0, "dsh_op_batch_metrics: dims must be positive");
    DSH_REQUIRE(joint_dim == 1 || joint_dim == 3, "dsh_op_batch_metrics: joint_dim must be 1 (per element) or 3 (per joint triplet)");
    DSH_REQUIRE(C % joint_dim == 0, "dsh_op_batch_metrics: channels must be a multiple of joint_dim");
    DSH_REQUIRE(b_div >= 2 && b_div <= B, "dsh_op_batch_metrics: b_div must be in 2 .. B (the pair mean of fewer than two clips divides by zero)");
    DSH_REQUIRE(b_div <= DV_MAX_BDIV, "dsh_op_batch_metrics: b_div is limited to 128 clips per diversity group");
    DSH_REQUIRE(((uintptr_t)result_dev % 8) == 0, "dsh_op_batch_metrics: result buffer must be 8-byte aligned");
    const long long clip_elems = (long long)T * C, n_elems = clip_elems * B, n_joints = n_elems / joint_dim;
    const int groups = B / b_div;
    const int n_chunks = (int)((clip_elems + DV_COLS - 1) / DV_COLS);
    double* res = reinterpret_cast<double*>(result_dev);
    double* part_sum = res + DSH_METRICS_HEADER + groups;
    long long* part_cnt = reinterpret_cast<long long*>(part_sum + MP_BLOCKS);
    double* part_div = part_sum + 2 * MP_BLOCKS;
    static bool attr = false;
    if (!attr) {
        DSH_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&diversity_partials), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          DV_MAX_BDIV * DV_COLS * (int)sizeof(float)));
        attr = true;
    }
    hipLaunchKernelGGL(mse_pck_partials, dim3(MP_BLOCKS), dim3(MP_THREADS), 0, s, outputs, motions, n_joints, joint_dim, part_sum, part_cnt);
    DSH_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(diversity_partials, dim3(n_chunks, groups), dim3(DV_COLS), (size_t)b_div * DV_COLS * sizeof(float), s, outputs,
                       clip_elems, b_div, n_chunks, part_div);
    DSH_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(metrics_finalize, dim3(1), dim3(64), 0, s, part_sum, part_cnt, part_div, n_chunks, groups, b_div, n_elems, n_joints,
                       clip_elems, res);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace dsh
