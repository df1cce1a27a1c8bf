// Forward kinematics of a rotation-only skeleton on the device: world-space joint positions (and world rotations) of the gesture
// channels, and the vector-Jacobian product of the positions with respect to the standardised axis-angle channels.
//
//   forward, per row r and joint j (parents[j] < j, parents[0] = -1):
//     v_i = x[r, 3i..] * std + mean                      i = joint_channel[j] >= 0: the joint is driven by channel triple i
//     R_j = exp([v_i]x) through the unit quaternion (sin(t/2)/t with 1/2 - t^2/48 below 1e-6, normalised: the route of rotation.hip)
//           | input kind "euler": deg = x * std + mean -> radians -> Rx Ry Rz
//           | rest_rot[j] where no channel drives the joint
//     W_0 = R_0,           p_0 = offsets[0]
//     W_j = W_parent R_j,  p_j = p_parent + W_parent offsets[j]
//   every 3-term product is (a0 b0 + a1 b1) + a2 b2.
//
//   vjp (axis-angle only), given g = dL/dpos: F_j = g_j, M_j = 0; then for j = J-1 .. 1 with p = parents[j] (a joint's children are
//   therefore added in descending index order, a fixed order):
//     M_p = M_p + (M_j + (p_j - p_p) x F_j),  F_p = F_p + F_j
//   which leaves M_j = sum over strict descendants k of (p_k - p_j) x g_k.  Per driven joint, u = W_j^T M_j and
//     dL/dv = (u + a (v x u)) + b (v x (v x u))        a = (1 - cos t)/t^2 = (sin(t/2)/(t/2))^2 / 2,  b = (t - sin t)/t^3
//     (below t = 1e-3: a = 1/2 - t^2/24, b = 1/6 - t^2/120),   dL/dx = std * dL/dv.
//   The forward pass is recomputed per row; nothing is saved between the two calls.
//
// Written from the mathematics, fp32 throughout, contraction to FMAs switched off, accurate sinf / cosf / sqrtf.
//
// Geometry: a block owns `blockDim.y` rows, one wave per row.  Lanes over the joints of the row build the local matrices into LDS; lane 0
// of the wave walks the joints in order, reading the parent's world matrix from LDS and overwriting the joint's local matrix with its
// world matrix (a walk with the matrices in registers would index them dynamically and spill); lanes over the row's outputs write them
// out contiguously.  Every value of a row is computed by one lane from that row's inputs and the skeleton alone, in an order that does
// not involve the block or grid size: no atomics, no cross-row reduction.  Rows behind a clip's length are never read and give zeros.
#include "dsh_kernels.h"

#pragma clang fp contract(off)

namespace dsh {

namespace {

constexpr int FK_LANES = 64;                     // lanes along the joints of a row (one wave)
constexpr int FK_MAX_ROWS_PER_BLOCK = 4;
constexpr size_t FK_LDS_BUDGET = 48 * 1024;      // bytes of LDS a block may ask for
constexpr int FK_FWD_FLOATS = 12;                // per joint and row: world matrix 9, position 3
constexpr int FK_VJP_FLOATS = 18;                // ... and force 3, moment 3
constexpr float FK_SMALL_ANGLE = 1e-6f;          // the quaternion's series threshold (rotation.hip)
constexpr float FK_SMALL_JR = 1e-3f;             // the series threshold of the right Jacobian's coefficients

__device__ inline float dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// axis-angle vector -> rotation matrix (row-major) through the normalised quaternion
__device__ inline void aa_matrix(float vx, float vy, float vz, float* R) {
    const float angle = sqrtf((vx * vx + vy * vy) + vz * vz);
    const float half = angle * 0.5f;
    const float k = fabsf(angle) < FK_SMALL_ANGLE ? 0.5f - (angle * angle) / 48.0f : sinf(half) / angle;
    const float r = cosf(half), i = vx * k, j = vy * k, q = vz * k;
    const float two_s = 2.0f / (((r * r + i * i) + j * j) + q * q);
    R[0] = 1.0f - two_s * (j * j + q * q); R[1] = two_s * (i * j - q * r);        R[2] = two_s * (i * q + j * r);
    R[3] = two_s * (i * j + q * r);        R[4] = 1.0f - two_s * (i * i + q * q); R[5] = two_s * (j * q - i * r);
    R[6] = two_s * (i * q - j * r);        R[7] = two_s * (j * q + i * r);        R[8] = 1.0f - two_s * (i * i + j * j);
}

// Euler XYZ in radians -> (Rx Ry) Rz, the composition of euler_to_axis_angle
__device__ inline void euler_matrix(float a, float b, float c, float* R) {
    const float sa = sinf(a), ca = cosf(a), sb = sinf(b), cb = cosf(b), sc = sinf(c), cc = cosf(c);
    const float a10 = sa * sb, a20 = -(ca * sb);
    R[0] = cb * cc;            R[1] = -(cb * sc);         R[2] = sb;
    R[3] = a10 * cc + ca * sc; R[4] = ca * cc - a10 * sc; R[5] = -(sa * cb);
    R[6] = a20 * cc + sa * sc; R[7] = sa * cc - a20 * sc; R[8] = ca * cb;
}

struct FkInput {
    const float* x; long long ldx; long long rows; int kind;
    const float* mean; const float* stdv; const int* lengths; int frames;
};

// the local matrices of one row into W[9 j ..], by the lanes of the row's wave
__device__ inline void fk_local(const FkSkeleton& sk, const FkInput& in, const float* xr, float* W, int lane) {
    const float PI_F = (float)3.14159265358979323846;
    for (int j = lane; j < sk.J; j += FK_LANES) {
        const int i = sk.joint_channel[j];
        float* R = W + 9 * j;
        if (i >= 0 && i < sk.Jc) {
            const int c = 3 * i;
            const float u0 = xr[c] * in.stdv[c] + in.mean[c];
            const float u1 = xr[c + 1] * in.stdv[c + 1] + in.mean[c + 1];
            const float u2 = xr[c + 2] * in.stdv[c + 2] + in.mean[c + 2];
            if (in.kind == 0) aa_matrix(u0, u1, u2, R);
            else euler_matrix(u0 * PI_F / 180.0f, u1 * PI_F / 180.0f, u2 * PI_F / 180.0f, R);
        } else {
            for (int e = 0; e < 9; ++e) R[e] = sk.rest_rot[9 * j + e];
        }
    }
}

__device__ inline int fk_parent(const FkSkeleton& sk, int j) {       // (contents are the caller's to validate; a bad entry stays inside the row)
    const int p = sk.parents[j];
    return p < 0 ? 0 : (p >= j ? j - 1 : p);
}

// one lane: local matrices in W -> world matrices in W, positions in P
__device__ inline void fk_walk(const FkSkeleton& sk, float* W, float* P) {
    P[0] = sk.offsets[0]; P[1] = sk.offsets[1]; P[2] = sk.offsets[2];
    for (int j = 1; j < sk.J; ++j) {
        const int p = fk_parent(sk, j);
        float w[9], r[9];
        for (int e = 0; e < 9; ++e) { w[e] = W[9 * p + e]; r[e] = W[9 * j + e]; }
        const float o0 = sk.offsets[3 * j], o1 = sk.offsets[3 * j + 1], o2 = sk.offsets[3 * j + 2];
        for (int a = 0; a < 3; ++a) {
            P[3 * j + a] = P[3 * p + a] + dot3(w[3 * a], w[3 * a + 1], w[3 * a + 2], o0, o1, o2);
            for (int b = 0; b < 3; ++b)
                W[9 * j + 3 * a + b] = dot3(w[3 * a], w[3 * a + 1], w[3 * a + 2], r[b], r[3 + b], r[6 + b]);
        }
    }
}

__device__ inline bool fk_padded(const FkInput& in, long long row) {
    return in.lengths != nullptr && (int)(row % in.frames) >= in.lengths[row / in.frames];
}

__global__ __launch_bounds__(FK_LANES * FK_MAX_ROWS_PER_BLOCK)
void fk_positions_kernel(FkInput in, FkSkeleton sk, float* pos, long long ld_pos, float* wrot, long long ld_wrot) {
    extern __shared__ float fk_lds[];
    const int lane = threadIdx.x, J = sk.J;
    float* W = fk_lds + (size_t)threadIdx.y * FK_FWD_FLOATS * J;
    float* P = W + 9 * J;
    const long long rows_per_pass = (long long)gridDim.x * blockDim.y;
    for (long long base = (long long)blockIdx.x * blockDim.y; base < in.rows; base += rows_per_pass) {     // block-uniform bounds
        const long long row = base + threadIdx.y;
        const bool active = row < in.rows;
        const bool live = active && !fk_padded(in, row);
        if (live) fk_local(sk, in, in.x + row * in.ldx, W, lane);
        __syncthreads();
        if (live && lane == 0) fk_walk(sk, W, P);
        __syncthreads();
        if (active) {
            float* pr = pos + row * ld_pos;
            for (int e = lane; e < 3 * J; e += FK_LANES) pr[e] = live ? P[e] : 0.0f;
            if (wrot) {
                float* wr = wrot + row * ld_wrot;
                for (int e = lane; e < 9 * J; e += FK_LANES) wr[e] = live ? W[e] : 0.0f;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(FK_LANES * FK_MAX_ROWS_PER_BLOCK)
void fk_positions_vjp_kernel(FkInput in, FkSkeleton sk, const float* g, long long ldg, float* dx, long long lddx) {
    extern __shared__ float fk_lds[];
    const int lane = threadIdx.x, J = sk.J;
    float* W = fk_lds + (size_t)threadIdx.y * FK_VJP_FLOATS * J;
    float* P = W + 9 * J;
    float* F = P + 3 * J;
    float* M = F + 3 * J;
    const long long rows_per_pass = (long long)gridDim.x * blockDim.y;
    for (long long base = (long long)blockIdx.x * blockDim.y; base < in.rows; base += rows_per_pass) {
        const long long row = base + threadIdx.y;
        const bool active = row < in.rows;
        const bool live = active && !fk_padded(in, row);
        const float* xr = in.x + row * in.ldx;
        if (live) {
            fk_local(sk, in, xr, W, lane);
            const float* gr = g + row * ldg;
            for (int e = lane; e < 3 * J; e += FK_LANES) { F[e] = gr[e]; M[e] = 0.0f; }
        }
        __syncthreads();
        if (live && lane == 0) {
            fk_walk(sk, W, P);
            for (int j = J - 1; j >= 1; --j) {
                const int p = fk_parent(sk, j);
                const float f0 = F[3 * j], f1 = F[3 * j + 1], f2 = F[3 * j + 2];
                const float d0 = P[3 * j] - P[3 * p], d1 = P[3 * j + 1] - P[3 * p + 1], d2 = P[3 * j + 2] - P[3 * p + 2];
                M[3 * p]     = M[3 * p]     + (M[3 * j]     + (d1 * f2 - d2 * f1));
                M[3 * p + 1] = M[3 * p + 1] + (M[3 * j + 1] + (d2 * f0 - d0 * f2));
                M[3 * p + 2] = M[3 * p + 2] + (M[3 * j + 2] + (d0 * f1 - d1 * f0));
                F[3 * p] = F[3 * p] + f0; F[3 * p + 1] = F[3 * p + 1] + f1; F[3 * p + 2] = F[3 * p + 2] + f2;
            }
        }
        __syncthreads();
        if (active) {
            float* dr = dx + row * lddx;
            for (int i = lane; i < sk.Jc; i += FK_LANES) {
                const int j = sk.channel_joint[i], c = 3 * i;
                float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
                if (live && j >= 0 && j < J) {
                    const float* w = W + 9 * j;
                    const float m0 = M[3 * j], m1 = M[3 * j + 1], m2 = M[3 * j + 2];
                    const float u0 = dot3(w[0], w[3], w[6], m0, m1, m2);       // W^T M
                    const float u1 = dot3(w[1], w[4], w[7], m0, m1, m2);
                    const float u2 = dot3(w[2], w[5], w[8], m0, m1, m2);
                    const float s0 = in.stdv[c], s1 = in.stdv[c + 1], s2 = in.stdv[c + 2];
                    const float v0 = xr[c] * s0 + in.mean[c], v1 = xr[c + 1] * s1 + in.mean[c + 1], v2 = xr[c + 2] * s2 + in.mean[c + 2];
                    const float t = sqrtf((v0 * v0 + v1 * v1) + v2 * v2);
                    float a, b;
                    if (t < FK_SMALL_JR) {
                        a = 0.5f - (t * t) / 24.0f;
                        b = 1.0f / 6.0f - (t * t) / 120.0f;
                    } else {
                        const float h = t * 0.5f, sh = sinf(h) / h;
                        a = 0.5f * (sh * sh);
                        b = (t - sinf(t)) / ((t * t) * t);
                    }
                    const float c0 = v1 * u2 - v2 * u1, c1 = v2 * u0 - v0 * u2, c2 = v0 * u1 - v1 * u0;           // v x u
                    const float e0 = v1 * c2 - v2 * c1, e1 = v2 * c0 - v0 * c2, e2 = v0 * c1 - v1 * c0;           // v x (v x u)
                    r0 = s0 * ((u0 + a * c0) + b * e0);
                    r1 = s1 * ((u1 + a * c1) + b * e1);
                    r2 = s2 * ((u2 + a * c2) + b * e2);
                }
                dr[c] = r0; dr[c + 1] = r1; dr[c + 2] = r2;
            }
        }
        __syncthreads();
    }
}

// rows per block (one wave each) and the block's LDS for `floats_per_joint` floats per joint and row
inline void fk_geometry(int J, int floats_per_joint, long long rows, dim3& grid, dim3& block, size_t& lds) {
    const size_t per_row = (size_t)floats_per_joint * J * sizeof(float);
    int rpb = (int)(FK_LDS_BUDGET / per_row);
    rpb = rpb < 1 ? 1 : (rpb > FK_MAX_ROWS_PER_BLOCK ? FK_MAX_ROWS_PER_BLOCK : rpb);
    const long long blocks = (rows + rpb - 1) / rpb;
    grid = dim3((unsigned)(blocks < 65536 ? blocks : 65536));
    block = dim3(FK_LANES, rpb);
    lds = per_row * rpb;
}

}  // namespace

int launch_fk_positions(const float* x, long long ldx, long long rows, int kind, const float* mean, const float* stdv, const FkSkeleton& sk,
                        float* pos, long long ld_pos, float* wrot, long long ld_wrot, const int* lengths, int frames, hipStream_t s) {
    if (rows == 0) return 0;
    dim3 grid, block;
    size_t lds;
    fk_geometry(sk.J, FK_FWD_FLOATS, rows, grid, block, lds);
    const FkInput in{x, ldx, rows, kind, mean, stdv, lengths, frames};
    hipLaunchKernelGGL(fk_positions_kernel, grid, block, lds, s, in, sk, pos, ld_pos, wrot, ld_wrot);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_fk_positions_vjp(const float* x, long long ldx, long long rows, const float* mean, const float* stdv, const FkSkeleton& sk,
                            const float* g, long long ldg, float* dx, long long lddx, const int* lengths, int frames, hipStream_t s) {
    if (rows == 0) return 0;
    dim3 grid, block;
    size_t lds;
    fk_geometry(sk.J, FK_VJP_FLOATS, rows, grid, block, lds);
    const FkInput in{x, ldx, rows, 0, mean, stdv, lengths, frames};
    hipLaunchKernelGGL(fk_positions_vjp_kernel, grid, block, lds, s, in, sk, g, ldg, dx, lddx);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace dsh
