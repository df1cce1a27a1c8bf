// BEAT results tail: axis-angle <-> Euler 'XYZ' conversion of the gesture channels, per joint triple, on the device.
//
//   axis_angle_to_euler   standardised axis-angle -> (standardised Euler degrees | plain degrees): what the reference saves, scores and
//                         writes to BVH (trainers/ddpm_beat_trainer.py:1044-1060, :1318-1333, :811-817):
//                           v = x std_aa + mean_aa -> quaternion (datasets/rotation_converter.py:204-233) -> the five matrix entries 'XYZ'
//                           reads (:251-280) -> Euler XYZ (:342-381) -> degrees -> (deg - mean_e) / std_e
//   euler_to_axis_angle   the dataset's direction (datasets/beat.py:376-401): deg = x std_e + mean_e -> radians -> Rx Ry Rz (:147-173) ->
//                         quaternion by the best-conditioned of four candidates (:44-103) -> axis-angle (:12-40) -> (aa - mean_aa) / std_aa
//
// Written from the mathematics, fp32 throughout, one rounded operation per operation of the reference's fp32 run (contraction to FMAs is
// switched off for this file, so the arithmetic does not depend on what the optimiser fuses), accurate sinf / cosf / atan2f / asinf / sqrtf.
// One deliberate deviation: the asin argument is clamped to [-1, 1].  At gimbal lock R02 can round an ulp past 1 and the reference's fp32
// run then returns NaN; here the middle angle is +-90 degrees.
//
// Geometry: one lane per joint triple, consecutive lanes on consecutive triples of a row (a wave reads one contiguous span), ROWS_PER_BLOCK
// rows per block, blocks stride over the rows.  Every triple is computed by exactly one lane from its own three inputs and the statistics:
// no reduction, no shared memory, so a result cannot depend on the launch geometry or on the other rows.
#include "dsh_kernels.h"

#pragma clang fp contract(off)

namespace dsh {

namespace {

constexpr int ROT_LANES = 64;           // lanes along the joints of a row (one wave)
constexpr int ROT_ROWS_PER_BLOCK = 4;
constexpr float SMALL_ANGLE = 1e-6f;    // rotation_converter.py:29, :219

// sin(a / 2) / a, with the series 1/2 - a^2 / 48 below the reference's threshold
__device__ inline float sin_half_over_angle(float half, float angle) {
    return fabsf(angle) < SMALL_ANGLE ? 0.5f - (angle * angle) / 48.0f : sinf(half) / angle;
}

// axis-angle vector -> Euler XYZ in radians
__device__ inline void aa_to_euler_xyz(float vx, float vy, float vz, float& ex, float& ey, float& ez) {
    const float angle = sqrtf(vx * vx + vy * vy + vz * vz);
    const float half = angle * 0.5f;
    const float k = sin_half_over_angle(half, angle);
    const float r = cosf(half), i = vx * k, j = vy * k, q = vz * k;
    const float two_s = 2.0f / (r * r + i * i + j * j + q * q);
    // R = I + two_s (...): only the entries 'XYZ' reads.  R = Rx(X) Ry(Y) Rz(Z) has R02 = sin Y, (R12, R22) = (-sin X, cos X) cos Y,
    // (R01, R00) = (-sin Z, cos Z) cos Y.
    const float r00 = 1.0f - two_s * (j * j + q * q);
    const float r01 = two_s * (i * j - q * r);
    const float r02 = two_s * (i * q + j * r);
    const float r12 = two_s * (j * q - i * r);
    const float r22 = 1.0f - two_s * (i * i + j * j);
    ex = atan2f(-r12, r22);
    ey = asinf(fminf(fmaxf(r02, -1.0f), 1.0f));       // the deviation: clamped, +-90 degrees instead of NaN
    ez = atan2f(-r01, r00);
}

// Euler XYZ in radians -> axis-angle vector
__device__ inline void euler_xyz_to_aa(float a, float b, float c, float& vx, float& vy, float& vz) {
    const float sa = sinf(a), ca = cosf(a), sb = sinf(b), cb = cosf(b), sc = sinf(c), cc = cosf(c);
    // (Rx Ry) Rz; the products with the 0 / 1 entries of the factors are exact
    const float a10 = sa * sb, a12 = -(sa * cb), a20 = -(ca * sb), a22 = ca * cb;
    const float m00 = cb * cc, m01 = -(cb * sc), m02 = sb;
    const float m10 = a10 * cc + ca * sc, m11 = ca * cc - a10 * sc, m12 = a12;
    const float m20 = a20 * cc + sa * sc, m21 = sa * cc - a20 * sc, m22 = a22;
    // |q| components from the diagonal (square roots of the positive parts), the candidate with the largest one
    const float t0 = 1.0f + m00 + m11 + m22, t1 = 1.0f + m00 - m11 - m22, t2 = 1.0f - m00 + m11 - m22, t3 = 1.0f - m00 - m11 + m22;
    const float q0 = t0 > 0.0f ? sqrtf(t0) : 0.0f, q1 = t1 > 0.0f ? sqrtf(t1) : 0.0f;
    const float q2 = t2 > 0.0f ? sqrtf(t2) : 0.0f, q3 = t3 > 0.0f ? sqrtf(t3) : 0.0f;
    int best = 0;
    float qb = q0;
    if (q1 > qb) { best = 1; qb = q1; }
    if (q2 > qb) { best = 2; qb = q2; }
    if (q3 > qb) { best = 3; qb = q3; }
    float w, x, y, z;                                  // the quaternion times 2 |q_best|
    if (best == 0)      { w = q0 * q0;   x = m21 - m12; y = m02 - m20; z = m10 - m01; }
    else if (best == 1) { w = m21 - m12; x = q1 * q1;   y = m10 + m01; z = m02 + m20; }
    else if (best == 2) { w = m02 - m20; x = m10 + m01; y = q2 * q2;   z = m12 + m21; }
    else                { w = m10 - m01; x = m20 + m02; y = m21 + m12; z = q3 * q3; }
    const float den = 2.0f * fmaxf(qb, 0.1f);
    w /= den; x /= den; y /= den; z /= den;
    // quaternion -> axis-angle; atan2 of (|xyz|, w) is above pi / 2 for w < 0: the angle is then above pi, as in the reference
    const float norm = sqrtf(x * x + y * y + z * z);
    const float half = atan2f(norm, w);
    const float angle = 2.0f * half;
    const float k = sin_half_over_angle(half, angle);
    vx = x / k; vy = y / k; vz = z / k;
}

// FORWARD: axis-angle -> Euler; else Euler -> axis-angle.  out_std: standardised result, out_raw: degrees (forward only); either may be null.
template <bool FORWARD>
__global__ __launch_bounds__(ROT_LANES * ROT_ROWS_PER_BLOCK)
void rotation_kernel(const float* x, long long ldx, long long rows, int joints, const float* mean_in, const float* std_in,
                     const float* mean_out, const float* std_out, float* out_std, long long ld_std, float* out_raw, long long ld_raw,
                     const int* lengths, int frames) {
    const float RAD2DEG = (float)(180.0 / 3.14159265358979323846), PI_F = (float)3.14159265358979323846;
    for (long long row = (long long)blockIdx.x * ROT_ROWS_PER_BLOCK + threadIdx.y; row < rows; row += (long long)gridDim.x * ROT_ROWS_PER_BLOCK) {
        const bool pad = lengths != nullptr && (int)(row % frames) >= lengths[row / frames];
        const float* xr = x + row * ldx;
        float* ys = out_std ? out_std + row * ld_std : nullptr;
        float* yr = out_raw ? out_raw + row * ld_raw : nullptr;
        for (int jt = threadIdx.x; jt < joints; jt += ROT_LANES) {
            const int c = 3 * jt;
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
            if (!pad) {                                 // a padded row is never read: whatever it holds, the result is 0
                const float u0 = xr[c] * std_in[c] + mean_in[c];
                const float u1 = xr[c + 1] * std_in[c + 1] + mean_in[c + 1];
                const float u2 = xr[c + 2] * std_in[c + 2] + mean_in[c + 2];
                if (FORWARD) {
                    aa_to_euler_xyz(u0, u1, u2, r0, r1, r2);
                    r0 *= RAD2DEG; r1 *= RAD2DEG; r2 *= RAD2DEG;
                } else {
                    euler_xyz_to_aa(u0 * PI_F / 180.0f, u1 * PI_F / 180.0f, u2 * PI_F / 180.0f, r0, r1, r2);
                }
                s0 = (r0 - mean_out[c]) / std_out[c];
                s1 = (r1 - mean_out[c + 1]) / std_out[c + 1];
                s2 = (r2 - mean_out[c + 2]) / std_out[c + 2];
            }
            if (ys) { ys[c] = s0; ys[c + 1] = s1; ys[c + 2] = s2; }
            if (yr) { yr[c] = r0; yr[c + 1] = r1; yr[c + 2] = r2; }
        }
    }
}

template <bool FORWARD>
int launch_rotation(const float* x, long long ldx, long long rows, int joints, const float* mean_in, const float* std_in,
                    const float* mean_out, const float* std_out, float* out_std, long long ld_std, float* out_raw, long long ld_raw,
                    const int* lengths, int frames, hipStream_t s) {
    if (rows == 0) return 0;
    const long long blocks = (rows + ROT_ROWS_PER_BLOCK - 1) / ROT_ROWS_PER_BLOCK;
    hipLaunchKernelGGL(rotation_kernel<FORWARD>, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(ROT_LANES, ROT_ROWS_PER_BLOCK), 0, s,
                       x, ldx, rows, joints, mean_in, std_in, mean_out, std_out, out_std, ld_std, out_raw, ld_raw, lengths, frames);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

int launch_axis_angle_to_euler(const float* x, long long ldx, long long rows, int joints, const float* mean_aa, const float* std_aa,
                               const float* mean_e, const float* std_e, float* y_std, long long ld_std, float* y_deg, long long ld_deg,
                               const int* lengths, int frames, hipStream_t s) {
    return launch_rotation<true>(x, ldx, rows, joints, mean_aa, std_aa, mean_e, std_e, y_std, ld_std, y_deg, ld_deg, lengths, frames, s);
}

int launch_euler_to_axis_angle(const float* x, long long ldx, long long rows, int joints, const float* mean_e, const float* std_e,
                               const float* mean_aa, const float* std_aa, float* y, long long ldy, const int* lengths, int frames,
                               hipStream_t s) {
    return launch_rotation<false>(x, ldx, rows, joints, mean_e, std_e, mean_aa, std_aa, y, ldy, nullptr, 0, lengths, frames, s);
}

}  // namespace dsh
