// Element-wise sampler updates (HBM-bound; one fused pass per step instead of the reference's ~10
// tiny aten kernels + H2D table copies per step, /root/reference/models/gaussian_diffusion.py):
//
//   ddim_step   x0 = c1 x - c2 eps; eps' = (c1 x - x0)/c2; x <- sqrt(ab_prev) x0 + sqrt(1-ab_prev) eps'
//               (+ RePaint blend)                                     :614-622, :993-1032, :1034-1056
//   undo_step   x <- sqrt(1-beta) x + sqrt(beta) n                   :464-473
//   ddpm_step   mean = coef1 x0 + coef2 x;  x <- mean + sigma n      :598-600, :747-773
//   q_sample    x <- sqrt(ab) x0 + sqrt(1-ab) n (n given, or drawn in the pass)  :434-462
//   guided      the DDIM / DPM2M / DDPM steps with the gradient of a per-column quadratic energy where the reference
//               uses its cond_fn (condition_score / condition_mean)  :645-682   (sibling kernels: guided_kernel)
//
// Every product / sum is an individually rounded fp32 op (rn_mul / rn_add / rn_sub of dsh_common.h: compiled with contraction off, so never fused into an FMA),
// in the reference's operation order, so the update itself is bit-identical to the aten sequence
// given identical inputs.  Scalars arrive pre-rounded exactly as the reference rounds them
// (fp64 table -> fp32 at gather, gaussian_diffusion.py:1514; sqrt taken in fp32 where the
// reference takes it on an fp32 tensor).
#include <algorithm>
#include <string>
#include <vector>

#include "dsh_common.h"
#include "dsh_kernels.h"

namespace dsh {

// torch.linspace(0, 1, L)[k] in fp32: symmetric formula start + step*k / end - step*(L-1-k).  The second half is ONE rounding in torch
// (its kernels are built with contraction on: end - step * m is an FMA), so it is an explicit fmaf here; with two roundings
// the weights differ from torch's at L = 10, 14, 15, 16, 18, ...
__device__ __forceinline__ float linspace01(int L, int k) {
    if (L == 1) return 0.f;
    const float step = __fdiv_rn(1.0f, (float)(L - 1));
    return (k < L / 2) ? rn_mul(step, (float)k) : fmaf(-step, (float)(L - 1 - k), 1.0f);
}

// What follows the update proper in both forms of the step: the RePaint select with its cross-fades on element i of the updated sample s,
// the store to x, and the saved noisy tail.
__device__ __forceinline__ void repaint_and_store(const DdimStepArgs& a, size_t i, int tc, float s) {
    const int t = (a.mask || a.tail_out) ? (int)((i % (size_t)tc) / (size_t)a.channels) : 0;
    if (a.mask) {
        // --same_overlap_noisy (gaussian_diffusion.py:1040-1042): the out-painted frames take the previous window's saved
        // NOISY tail of this level instead of a freshly noised copy of its final tail (no Gaussian draw in that branch)
        float g;
        if (a.tail_in) {
            const size_t b = i / (size_t)tc;
            const int c = (int)(i % (size_t)a.channels);
            g = t < a.overlap_len ? a.tail_in[(b * a.overlap_len + t) * a.channels + c] : a.gt[i];
        } else g = rn_add(rn_mul(a.sqrt_ab_prev, a.gt[i]), rn_mul(a.sqrt_1m_ab_prev, a.noise2[i]));
        if (a.blend) {
            const int L = a.overlap_len;
            if (t < L) {
                const float w = linspace01(L, t);
                g = rn_add(rn_mul(g, rn_sub(1.0f, w)), rn_mul(s, w));
            } else if (a.tail_blend && t >= a.frames - L) {
                // mirrored fade of a window pinned at both ends: the head's weights in reverse order (the same fp32 values),
                // w'[j] = linspace(0, 1, L)[L - 1 - j], j = t - (frames - L); disjoint from the head's frames (2 L <= frames)
                const float w = linspace01(L, L - 1 - (t - (a.frames - L)));
                g = rn_add(rn_mul(g, rn_sub(1.0f, w)), rn_mul(s, w));
            }
        }
        s = a.mask[i] ? g : s;
    }
    a.x[i] = s;
    if (a.tail_out && t >= a.frames - a.overlap_len) {          // saved_noisy_tail[t] = x[..., -L:, :]  (:1058-1060)
        const size_t b = i / (size_t)tc;
        const int c = (int)(i % (size_t)a.channels);
        a.tail_out[(b * a.overlap_len + (t - (a.frames - a.overlap_len))) * a.channels + c] = s;
    }
}

// SECOND: DPM-Solver++(2M), data prediction, at eta = 0 (Lu et al. 2022, algorithm 2): the second-order multistep update
//   x0 = c1 x - c2 eps;  D = x0 + G (x0 - x0_prev);  x <- A x + Bc D
// with A = sigma_prev / sigma, Bc = -alpha_prev expm1(-h), G = h / (2 h_before) from the host (sampler.hip, solver_coeffs).  x0_prev
// (in x0_out) is read and rewritten by the thread that owns the element.
template <bool SECOND>
__global__ void ddim_step_kernel(DdimStepArgs a) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int tc = a.frames * a.channels;
    const bool ranged = a.c_hi > a.c_lo;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        if (ranged) { const int cc = (int)(i % (size_t)a.channels); if (cc < a.c_lo || cc >= a.c_hi) continue; }
        const float x = a.x[i];
        const float e = a.eps[i];
        const float c1x = rn_mul(a.c1, x);
        float x0 = rn_sub(c1x, rn_mul(a.c2, e));
        if (a.clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
        float s;
        if (SECOND) {
            const float D = rn_add(x0, rn_mul(a.G, rn_sub(x0, a.x0_out[i])));
            s = rn_add(rn_mul(a.A, x), rn_mul(a.Bc, D));
            a.x0_out[i] = x0;
        } else {
            const float e2 = __fdiv_rn(rn_sub(c1x, x0), a.c2);
            s = rn_add(rn_mul(x0, a.sqrt_ab_prev), rn_mul(a.coef_eps, e2));
            if (a.noise1) s = rn_add(s, rn_mul(a.sigma, a.noise1[i]));
            if (a.x0_out) a.x0_out[i] = x0;
        }
        repaint_and_store(a, i, tc, s);
    }
}

static inline int grid_for(size_t n) {
    size_t b = (n + 255) / 256;
    return (int)(b < 2048 ? (b ? b : 1) : 2048);
}

int launch_ddim_step(const DdimStepArgs& a, hipStream_t s) {
    if (a.second) {
        DSH_REQUIRE(a.x && a.eps && a.x0_out && a.frames > 0 && a.channels > 0, "dpm2m_step: invalid argument");
        DSH_REQUIRE(!a.noise1 && !a.tail_in && !a.tail_out, "dpm2m_step: no eta draw and no saved noisy tails");
        DSH_REQUIRE(!a.mask || (a.gt && a.noise2), "dpm2m_step: a mask needs gt and noise2");
        DSH_REQUIRE(a.c_lo >= 0 && a.c_hi <= a.channels, "dpm2m_step: channel range outside [0, channels]");
        if (a.n == 0) return 0;
        hipLaunchKernelGGL(ddim_step_kernel<true>, dim3(grid_for(a.n)), dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL(ddim_step_kernel<false>, dim3(grid_for(a.n)), dim3(256), 0, s, a);
    }
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ void undo_step_kernel(float* x, const float* noise, float sa, float sb, size_t n, int channels, int c_lo, int c_hi) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const bool ranged = c_hi > c_lo;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (ranged) { const int cc = (int)(i % (size_t)channels); if (cc < c_lo || cc >= c_hi) continue; }
        x[i] = rn_add(rn_mul(sa, x[i]), rn_mul(sb, noise[i]));
    }
}
int launch_undo_step(float* x, const float* noise, float sqrt_1m_beta, float sqrt_beta, size_t n, hipStream_t s, int channels, int c_lo, int c_hi) {
    DSH_REQUIRE(c_hi <= c_lo || channels > 0, "undo_step: a channel range needs the channel count");
    hipLaunchKernelGGL(undo_step_kernel, dim3(grid_for(n)), dim3(256), 0, s, x, noise, sqrt_1m_beta, sqrt_beta, n, channels, c_lo, c_hi);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ void ddpm_step_kernel(DdpmStepArgs a) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const bool ranged = a.c_hi > a.c_lo;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        if (ranged) { const int cc = (int)(i % (size_t)a.channels); if (cc < a.c_lo || cc >= a.c_hi) continue; }
        const float x = a.x[i];
        float x0 = rn_sub(rn_mul(a.c1, x), rn_mul(a.c2, a.eps[i]));
        if (a.clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
        const float mean = rn_add(rn_mul(a.coef1, x0), rn_mul(a.coef2, x));
        if (a.x0_out) a.x0_out[i] = x0;
        // reference: mean + nonzero_mask * exp(0.5*logvar) * noise  (left-to-right products)
        a.x[i] = rn_add(mean, rn_mul(a.sigma, a.noise[i]));
    }
}
int launch_ddpm_step(const DdpmStepArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(ddpm_step_kernel, dim3(grid_for(a.n)), dim3(256), 0, s, a);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- guided steps: soft constraints while sampling (dsh_kernels.h, GuideArgs) ----
// g[t] from z at t-2 .. t+2 of one column of a clip of L frames (values at frames outside [0, L) are not read: their predicates are false):
//   g = -scale (W (z - Y) + vel ([t>=1] v[t-1] - [t<=L-2] v[t]) + acc ([2<=t] a[t-1] - 2 [1<=t<=L-2] a[t] + [t<=L-3] a[t+1]))
// with v[t] = z[t+1] - z[t], a[t] = (z[t+1] - 2 z[t]) + z[t-1]; every product and sum rounded on its own, in this order.
__device__ __forceinline__ float guide_grad(const GuideArgs& g, size_t i, int t, int L, float lv, float la, float zm2, float zm1, float z0,
                                            float zp1, float zp2) {
    float sum = 0.f;
    if (g.weight) sum = rn_mul(g.weight[i], rn_sub(z0, g.target ? g.target[i] : 0.f));
    if (g.vel) {
        const float vm = t >= 1 ? rn_sub(z0, zm1) : 0.f;
        const float v0 = t <= L - 2 ? rn_sub(zp1, z0) : 0.f;
        sum = rn_add(sum, rn_mul(lv, rn_sub(vm, v0)));
    }
    if (g.acc) {
        const float am = t >= 2 ? rn_add(rn_sub(z0, rn_mul(2.0f, zm1)), zm2) : 0.f;
        const float a0 = (t >= 1 && t <= L - 2) ? rn_add(rn_sub(zp1, rn_mul(2.0f, z0)), zm1) : 0.f;
        const float ap = t <= L - 3 ? rn_add(rn_sub(zp2, rn_mul(2.0f, zp1)), z0) : 0.f;
        sum = rn_add(sum, rn_mul(la, rn_add(rn_sub(am, rn_mul(2.0f, a0)), ap)));
    }
    return -rn_mul(g.scale, sum);
}

struct GuidedKernelArgs {
    DdimStepArgs d;        // GUIDED_DDIM / GUIDED_DPM2M
    DdpmStepArgs p;        // GUIDED_DDPM
    const float* z; float* g_out;      // GUIDED_GRAD
    GuideArgs g;
    size_t cols;           // B * channels: one thread per column of a clip
    int frames, channels, c_lo, c_hi;
};
enum GuidedMode { GUIDED_GRAD = 0, GUIDED_DDIM = 1, GUIDED_DPM2M = 2, GUIDED_DDPM = 3 };

// Lanes run across the columns of a frame (coalesced rows); each lane walks ALL frames of its column of its clip with z at t-2 .. t+2 and
// x / eps at t .. t+2 in registers.  The steps update x in place, so a column is one thread's: it has read frame t + 2 before it stores
// frame t, and nothing else reads or writes that column (a frame chunk per thread would read halo frames its neighbour is storing).
// No LDS, no atomics; a clip's result depends on its own column, its length and the launch's scalars only.
// X0: z is pred_xstart = clip(c1 x - c2 eps), re-derived for the neighbouring frames from their x and eps.
template <int MODE, bool X0>
__global__ void guided_kernel(GuidedKernelArgs a) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int T = a.frames, C = a.channels;
    const bool ranged = a.c_hi > a.c_lo;
    const float* xs = MODE == GUIDED_GRAD ? a.z : MODE == GUIDED_DDPM ? a.p.x : a.d.x;
    const float* es = MODE == GUIDED_GRAD ? nullptr : MODE == GUIDED_DDPM ? a.p.eps : a.d.eps;
    const float c1 = MODE == GUIDED_DDPM ? a.p.c1 : a.d.c1, c2 = MODE == GUIDED_DDPM ? a.p.c2 : a.d.c2;
    const int clip = MODE == GUIDED_DDPM ? a.p.clip : a.d.clip;
    const int tc = T * C;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.cols; j += stride) {
        const size_t b = j / (size_t)C;
        const int c = (int)(j - b * (size_t)C);
        if (ranged && (c < a.c_lo || c >= a.c_hi)) continue;
        int L = a.g.lens ? a.g.lens[b] : T;
        L = L < 0 ? 0 : (L > T ? T : L);
        const size_t base = b * (size_t)tc + (size_t)c;
        const float lv = a.g.vel ? a.g.vel[c] : 0.f, la = a.g.acc ? a.g.acc[c] : 0.f;
        // frame t of the column (t < L): x, eps and the guided signal
        auto load = [&](int t, float& x, float& e, float& z) {
            const size_t i = base + (size_t)t * C;
            x = xs[i];
            e = MODE == GUIDED_GRAD ? 0.f : es[i];
            if (MODE != GUIDED_GRAD && X0) {
                z = rn_sub(rn_mul(c1, x), rn_mul(c2, e));
                if (clip) z = fminf(fmaxf(z, -1.0f), 1.0f);
            } else z = x;
        };
        float zm2 = 0.f, zm1 = 0.f, z0 = 0.f, z1 = 0.f, z2 = 0.f, x0 = 0.f, x1 = 0.f, x2 = 0.f, e0 = 0.f, e1 = 0.f, e2 = 0.f;
        if (L > 0) load(0, x0, e0, z0);
        if (L > 1) load(1, x1, e1, z1);
        for (int t = 0; t < L; ++t) {
            x2 = e2 = z2 = 0.f;
            if (t + 2 < L) load(t + 2, x2, e2, z2);
            const size_t i = base + (size_t)t * C;
            const float g = guide_grad(a.g, i, t, L, lv, la, zm2, zm1, z0, z1, z2);
            if (MODE == GUIDED_GRAD) {
                a.g_out[i] = g;
            } else if (MODE == GUIDED_DDPM) {
                float p0 = rn_sub(rn_mul(c1, x0), rn_mul(c2, e0));
                if (clip) p0 = fminf(fmaxf(p0, -1.0f), 1.0f);
                float mean = rn_add(rn_mul(a.p.coef1, p0), rn_mul(a.p.coef2, x0));
                if (g != 0.f) mean = rn_add(mean, rn_mul(a.g.post_var, g));      // condition_mean: mean + variance * gradient
                if (a.p.x0_out) a.p.x0_out[i] = p0;
                a.p.x[i] = rn_add(mean, rn_mul(a.p.sigma, a.p.noise[i]));
            } else {
                const float c1x = rn_mul(c1, x0);
                float p0 = rn_sub(c1x, rn_mul(c2, e0));
                if (clip) p0 = fminf(fmaxf(p0, -1.0f), 1.0f);
                // condition_score: eps re-derived from pred_xstart, shifted, and pred_xstart re-derived from it (not clipped again)
                // (an element whose gradient is exactly 0 — no term touches it, or a zero scale — takes the parent's update bit for bit: the
                //  round trip through eps would move its last bits for nothing)
                const float eg = rn_sub(__fdiv_rn(rn_sub(c1x, p0), c2), rn_mul(a.g.sqrt_1m_ab, g));
                const float pg = g == 0.f ? p0 : rn_sub(c1x, rn_mul(c2, eg));
                float s;
                if (MODE == GUIDED_DPM2M) {
                    const float D = rn_add(pg, rn_mul(a.d.G, rn_sub(pg, a.d.x0_out[i])));
                    s = rn_add(rn_mul(a.d.A, x0), rn_mul(a.d.Bc, D));
                    a.d.x0_out[i] = pg;
                } else {
                    const float en = __fdiv_rn(rn_sub(c1x, pg), c2);
                    s = rn_add(rn_mul(pg, a.d.sqrt_ab_prev), rn_mul(a.d.coef_eps, en));
                    if (a.d.noise1) s = rn_add(s, rn_mul(a.d.sigma, a.d.noise1[i]));
                    if (a.d.x0_out) a.d.x0_out[i] = pg;
                }
                repaint_and_store(a.d, b * (size_t)tc + (size_t)t * C + (size_t)c, tc, s);
            }
            zm2 = zm1; zm1 = z0; z0 = z1; z1 = z2;
            x0 = x1; x1 = x2; e0 = e1; e1 = e2;
        }
        // GUIDED_GRAD: frames beyond the clip's length get gradient 0; the steps leave them as they are
        if (MODE == GUIDED_GRAD) for (int t = L; t < T; ++t) a.g_out[base + (size_t)t * C] = 0.f;
    }
}

static int check_guide(const GuideArgs& g, int B, int frames, int channels, int c_lo, int c_hi, const char* what) {
    DSH_REQUIRE(B > 0 && frames > 0 && channels > 0, std::string(what) + ": invalid argument");
    DSH_REQUIRE(c_lo >= 0 && c_hi <= channels, std::string(what) + ": channel range outside [0, channels]");
    DSH_REQUIRE(g.space == GUIDE_XT || g.space == GUIDE_X0, std::string(what) + ": unknown guidance space (0 x_t, 1 x0)");
    return 0;
}
template <int MODE>
static int launch_guided(GuidedKernelArgs& k, int B, hipStream_t s) {
    k.cols = (size_t)B * k.channels;
    const dim3 grid(grid_for(k.cols)), block(256);
    if (k.g.space == GUIDE_X0) hipLaunchKernelGGL((guided_kernel<MODE, true>), grid, block, 0, s, k);
    else hipLaunchKernelGGL((guided_kernel<MODE, false>), grid, block, 0, s, k);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_guidance_grad(const float* z, float* g, int B, int frames, int channels, int c_lo, int c_hi, const GuideArgs& ga, hipStream_t s) {
    if (int e = check_guide(ga, B, frames, channels, c_lo, c_hi, "guidance_grad")) return e;
    DSH_REQUIRE(z && g && z != g, "guidance_grad: null pointer (or g aliases z)");
    GuidedKernelArgs k{};
    k.z = z; k.g_out = g; k.g = ga; k.g.space = GUIDE_XT;       // (z is given: nothing to re-derive)
    k.frames = frames; k.channels = channels; k.c_lo = c_lo; k.c_hi = c_hi;
    return launch_guided<GUIDED_GRAD>(k, B, s);
}

int launch_guided_ddim_step(const DdimStepArgs& a, const GuideArgs& ga, hipStream_t s) {
    DSH_REQUIRE(a.x && a.eps && a.frames > 0 && a.channels > 0, "guided_ddim_step: invalid argument");
    const size_t row = (size_t)a.frames * a.channels;
    DSH_REQUIRE(a.n > 0 && a.n % row == 0, "guided_ddim_step: the element count is not a whole number of clips");
    const int B = (int)(a.n / row);
    if (int e = check_guide(ga, B, a.frames, a.channels, a.c_lo, a.c_hi, "guided_ddim_step")) return e;
    DSH_REQUIRE(!a.mask || a.tail_in || (a.gt && a.noise2), "guided_ddim_step: a mask needs gt and noise2");
    if (a.second) {
        DSH_REQUIRE(a.x0_out, "guided_ddim_step: the second-order step needs the x0 history");
        DSH_REQUIRE(!a.noise1 && !a.tail_in && !a.tail_out, "guided_ddim_step: second order: no eta draw and no saved noisy tails");
    }
    GuidedKernelArgs k{};
    k.d = a; k.g = ga; k.frames = a.frames; k.channels = a.channels; k.c_lo = a.c_lo; k.c_hi = a.c_hi;
    return a.second ? launch_guided<GUIDED_DPM2M>(k, B, s) : launch_guided<GUIDED_DDIM>(k, B, s);
}

int launch_guided_ddpm_step(const DdpmStepArgs& a, int frames, const GuideArgs& ga, hipStream_t s) {
    DSH_REQUIRE(a.x && a.eps && a.noise && frames > 0 && a.channels > 0, "guided_ddpm_step: invalid argument");
    const size_t row = (size_t)frames * a.channels;
    DSH_REQUIRE(a.n > 0 && a.n % row == 0, "guided_ddpm_step: the element count is not a whole number of clips");
    const int B = (int)(a.n / row);
    if (int e = check_guide(ga, B, frames, a.channels, a.c_lo, a.c_hi, "guided_ddpm_step")) return e;
    GuidedKernelArgs k{};
    k.p = a; k.g = ga; k.frames = frames; k.channels = a.channels; k.c_lo = a.c_lo; k.c_hi = a.c_hi;
    return launch_guided<GUIDED_DDPM>(k, B, s);
}

__global__ void fill_i64_kernel(int64_t* p, int64_t v, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
int launch_fill_i64(int64_t* p, int64_t v, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(fill_i64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, v, n);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}
__global__ void fill_f32_kernel(float* p, float v, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
int launch_fill_f32(float* p, float v, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(fill_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, v, n);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}
// host values -> device in stream order without a host sync: 64 values per launch travel as the kernel's by-value argument
struct F32x64 { float v[64]; };
__global__ void store_values_kernel(float* p, F32x64 v, int n) {
    if ((int)threadIdx.x < n) p[threadIdx.x] = v.v[threadIdx.x];
}
int launch_store_values_f32(float* p, const float* host, int n, hipStream_t s) {
    for (int i = 0; i < n; i += 64) {
        F32x64 v{};
        const int k = std::min(64, n - i);
        for (int j = 0; j < k; ++j) v.v[j] = host[i + j];
        hipLaunchKernelGGL(store_values_kernel, dim3(1), dim3(64), 0, s, p + i, v, k);
        DSH_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

// one launch for the per-step scalars of an evaluation: t, the two x0 coefficients and the spaced level (timestep-cache slot)
__global__ void fill_step_kernel(int64_t* t, float* c1, float* c2, int64_t* level, int64_t tv, float c1v, float c2v, int64_t lv, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { t[i] = tv; c1[i] = c1v; c2[i] = c2v; }
    if (i == 0) *level = lv;
}
int launch_fill_step(int64_t* t, float* c1, float* c2, int64_t* level, int64_t tv, float c1v, float c2v, int64_t lv, int n, hipStream_t s) {
    hipLaunchKernelGGL(fill_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t, c1, c2, level, tv, c1v, c2v, lv, n);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// save (restore == 0) / restore the x-independent results of one evaluation to / from timestep-cache slot *level: up to four
// byte ranges (multiples of 16) of the workspace <-> slots + *level * stride + off[seg]
__global__ void level_copy_kernel(LevelCopyArgs a) {
    char* slot = a.slots + (size_t)(*a.level) * a.stride;
    const size_t stride = (size_t)gridDim.x * blockDim.x * 16;
    for (int sg = 0; sg < a.nseg; ++sg) {
        char* w = a.work[sg];
        char* c = slot + a.off[sg];
        for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 16; i < a.bytes[sg]; i += stride) {
            if (a.restore) *reinterpret_cast<uint4*>(w + i) = *reinterpret_cast<const uint4*>(c + i);
            else *reinterpret_cast<uint4*>(c + i) = *reinterpret_cast<const uint4*>(w + i);
        }
    }
}
int launch_level_copy(const LevelCopyArgs& a, hipStream_t s) {
    size_t mx = 0;
    for (int i = 0; i < a.nseg; ++i) { DSH_REQUIRE(a.bytes[i] % 16 == 0 && a.off[i] % 16 == 0, "level_copy: ranges must be 16-byte multiples"); mx = std::max(mx, a.bytes[i]); }
    const size_t blocks = std::min<size_t>(std::max<size_t>((mx / 16 + 255) / 256, 1), 1024);
    hipLaunchKernelGGL(level_copy_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- Philox4x32-10 counter RNG + Box-Muller (perf runs; parity runs inject recorded noise) ------
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

// row_keys == null: one stream for the whole tensor (key `seed`, counter offset + quad index).
// row_keys != null: row b (= n_row consecutive values, n_row % 4 == 0) is its own stream: same key `seed`, the row key in the two
// HIGH words of the 128-bit Philox counter (they are zero in the whole-tensor mode) and the counter offset + quad index INSIDE
// the row in the low words — so a chain's noise does not depend on which batch / rank it is sampled in, and two (seed, row key)
// pairs share a stream only if both components are equal (round 2 XORed the row key into the seed: (s + 1) ^ 0 == s ^ 1).
// row_lens != null (ragged batch, with row_keys): row b holds row_lens[b] valid frames of `channels` values in front of its padding and
// advances by ITS OWN size per draw — counter = draw * (row_lens[b] * channels / 4) + quad index inside the row — which is the stream the
// clip draws from when it is sampled alone at that length.  (Padded positions run on into the next draw's counters; nothing reads them.)
// row_seeds != null (with row_keys): row b uses the Philox key row_seeds[b] in place of `seed`; counter and row key as above — rows of one
// batch may then stand at different windows of their chains (key = hash(base seed, window index), live sessions batched together).
// the four N(0,1) values of quad `qd` of a draw (addressing above): shared by the stand-alone draw and the fused q_sample pass
__device__ __forceinline__ void philox_quad(size_t qd, uint64_t seed, uint64_t offset, const uint64_t* __restrict__ row_keys, size_t row_quads,
                                            const int* __restrict__ row_lens, uint64_t draw, int channels,
                                            const uint64_t* __restrict__ row_seeds, float (&z)[4]) {
    uint64_t ctr = offset + qd, rk = 0;
    uint64_t key = seed;
    if (row_keys) {
        const size_t b = qd / row_quads;
        if (row_seeds) key = row_seeds[b];
        ctr = (row_lens ? draw * ((uint64_t)row_lens[b] * (uint64_t)channels / 4) : offset) + (qd - b * row_quads);
        rk = row_keys[b];
    }
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)rk, (uint32_t)(rk >> 32)};
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = ((float)(c[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);      // (0,1)
        const float u2 = ((float)(c[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float r = sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincosf(6.283185307179586f * u2, &sn, &cs);
        z[2 * h] = r * cs;
        z[2 * h + 1] = r * sn;
    }
}
__global__ void philox_randn_kernel(float* out, size_t n, uint64_t seed, uint64_t offset, const uint64_t* __restrict__ row_keys,
                                    size_t row_quads, const int* __restrict__ row_lens, uint64_t draw, int channels,
                                    const uint64_t* __restrict__ row_seeds) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t nquad = (n + 3) / 4;
    for (size_t qd = (size_t)blockIdx.x * blockDim.x + threadIdx.x; qd < nquad; qd += stride) {
        float z[4];
        philox_quad(qd, seed, offset, row_keys, row_quads, row_lens, draw, channels, row_seeds, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t i = qd * 4 + j;
            if (i < n) out[i] = z[j];
        }
    }
}
int launch_philox_randn(float* out, size_t n, uint64_t seed, uint64_t offset, hipStream_t s) {
    hipLaunchKernelGGL(philox_randn_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, s, out, n, seed, offset,
                       (const uint64_t*)nullptr, (size_t)1, (const int*)nullptr, (uint64_t)0, 0, (const uint64_t*)nullptr);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_philox_randn_rows(float* out, int rows, size_t n_row, uint64_t seed, uint64_t offset, const uint64_t* row_keys,
                             hipStream_t s, const int* row_lens, uint64_t draw, int channels, const uint64_t* row_seeds) {
    DSH_REQUIRE(rows > 0 && n_row % 4 == 0 && row_keys, "philox_randn_rows: row length must be a multiple of 4");
    DSH_REQUIRE(!row_lens || channels > 0, "philox_randn_rows: per-row lengths need the channel count");
    const size_t n = (size_t)rows * n_row;
    hipLaunchKernelGGL(philox_randn_kernel, dim3(grid_for(n / 4)), dim3(256), 0, s, out, n, seed, offset, row_keys, n_row / 4, row_lens, draw, channels, row_seeds);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- q_sample: out = a_b x0 + s_b n, one coefficient pair per batch row (gaussian_diffusion.py:434-462) ----
// n is the caller's (a.noise) or drawn here, quad by quad, with the addressing of philox_randn_kernel: one pass, no noise buffer.  Columns
// outside [c_lo, c_hi) (c_hi > c_lo) are not written; columns >= fixed_from (fixed_from >= 0) are copied from x0 (fix_head_var, :443-456:
// coefficient pair 1 / 0 there); ragged rows (row_lens, with the row keys) write 0 to their padded frames.  out may be x0 (every element is
// read before it is written, by the thread that writes it).
__global__ void q_sample_kernel(QSampleArgs a) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t nquad = (a.n + 3) / 4, row_n = (size_t)a.frames * a.channels;
    const bool ranged = a.c_hi > a.c_lo;
    for (size_t qd = (size_t)blockIdx.x * blockDim.x + threadIdx.x; qd < nquad; qd += stride) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (!a.noise) philox_quad(qd, a.seed, a.offset, a.row_keys, a.row_quads, a.row_lens, a.draw, a.channels, a.row_seeds, z);
        if (a.vec) {
            // (launch_q_sample: every quad lies inside one row, all columns are written alike, the pointers are 16-byte aligned)
            const size_t b = qd * 4 / row_n;
            const float ca = a.a[b], cs = a.s[b];
            const float4 x0 = *reinterpret_cast<const float4*>(a.x0 + qd * 4);
            if (a.noise) { const float4 n = *reinterpret_cast<const float4*>(a.noise + qd * 4); z[0] = n.x; z[1] = n.y; z[2] = n.z; z[3] = n.w; }
            float4 o;
            o.x = rn_add(rn_mul(ca, x0.x), rn_mul(cs, z[0])); o.y = rn_add(rn_mul(ca, x0.y), rn_mul(cs, z[1]));
            o.z = rn_add(rn_mul(ca, x0.z), rn_mul(cs, z[2])); o.w = rn_add(rn_mul(ca, x0.w), rn_mul(cs, z[3]));
            *reinterpret_cast<float4*>(a.out + qd * 4) = o;
            continue;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t i = qd * 4 + j;
            if (i >= a.n) break;
            const size_t b = i / row_n, in_row = i - b * row_n;
            const int cc = (int)(in_row % (size_t)a.channels);
            if (ranged && (cc < a.c_lo || cc >= a.c_hi)) continue;
            if (a.row_lens && in_row / (size_t)a.channels >= (size_t)a.row_lens[b]) { a.out[i] = 0.f; continue; }
            const float x0 = a.x0[i];
            if (a.fixed_from >= 0 && cc >= a.fixed_from) { a.out[i] = x0; continue; }
            const float nz = a.noise ? a.noise[i] : z[j];
            a.out[i] = rn_add(rn_mul(a.a[b], x0), rn_mul(a.s[b], nz));
        }
    }
}
int launch_q_sample(const QSampleArgs& a, hipStream_t s) {
    DSH_REQUIRE(a.out && a.x0 && a.a && a.s && a.frames > 0 && a.channels > 0, "q_sample: invalid argument");
    DSH_REQUIRE(a.n % ((size_t)a.frames * a.channels) == 0, "q_sample: the element count is not a whole number of rows");
    DSH_REQUIRE(a.c_lo >= 0 && a.c_hi <= a.channels, "q_sample: channel range outside [0, channels]");
    DSH_REQUIRE(a.noise || !a.row_keys || (a.row_quads > 0 && a.row_quads * 4 == (size_t)a.frames * a.channels), "q_sample: row keys need frames * channels to be a multiple of 4");
    DSH_REQUIRE(!a.row_lens || a.noise || a.row_keys, "q_sample: per-row lengths of a Philox draw need the row keys");
    if (a.n == 0) return 0;
    QSampleArgs v = a;
    auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    v.vec = a.c_hi <= a.c_lo && a.fixed_from < 0 && !a.row_lens && ((size_t)a.frames * a.channels) % 4 == 0 && aligned(a.out) && aligned(a.x0) &&
            (!a.noise || aligned(a.noise)) ? 1 : 0;
    hipLaunchKernelGGL(q_sample_kernel, dim3(grid_for((a.n + 3) / 4)), dim3(256), 0, s, v);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- keep mask of an edit: keep[b, t, c] = 0 where frame t lies in one of row b's nf frame ranges or column c in one of the nc column
// ranges, 1 elsewhere.  frames [B, nf, 2] / cols [nc, 2] (device int32, half-open).  The host validates the ranges before the launch; a
// range outside [0, T] / [0, C] or with lo > hi is skipped all the same.
__global__ void region_mask_kernel(const int* __restrict__ frames, int nf, const int* __restrict__ cols, int nc, size_t n, int T, int C,
                                   uint8_t* __restrict__ keep) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, row_n = (size_t)T * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const size_t b = i / row_n, in_row = i - b * row_n;
        const int t = (int)(in_row / C), c = (int)(in_row - (size_t)t * C);
        bool edit = false;
        for (int j = 0; j < nf; ++j) {
            const int lo = frames[(b * nf + j) * 2], hi = frames[(b * nf + j) * 2 + 1];
            if (lo >= 0 && hi <= T && lo <= hi && t >= lo && t < hi) edit = true;
        }
        for (int j = 0; j < nc; ++j) {
            const int lo = cols[2 * j], hi = cols[2 * j + 1];
            if (lo >= 0 && hi <= C && lo <= hi && c >= lo && c < hi) edit = true;
        }
        keep[i] = edit ? 0 : 1;
    }
}
int launch_region_mask(const int* frames, int nf, const int* cols, int nc, int B, int T, int C, uint8_t* keep, hipStream_t s) {
    DSH_REQUIRE(B >= 0 && T > 0 && C > 0 && nf >= 0 && nc >= 0, "region_mask: invalid argument");
    if (B == 0) return 0;
    DSH_REQUIRE(keep && (nf == 0 || frames) && (nc == 0 || cols), "region_mask: null pointer");
    const size_t n = (size_t)B * T * C;
    hipLaunchKernelGGL(region_mask_kernel, dim3(grid_for(n)), dim3(256), 0, s, frames, nf, cols, nc, n, T, C, keep);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// ragged batch: x[b, t, :] = 0 for t >= lens[b] (the padded frames of a sampling loop's result)
__global__ void zero_padded_frames_kernel(float* __restrict__ x, const int* __restrict__ lens, size_t n, int frames, int channels) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, row_n = (size_t)frames * channels;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const size_t b = i / row_n;
        if ((i - b * row_n) / channels >= (size_t)lens[b]) x[i] = 0.f;
    }
}
int launch_zero_padded_frames(float* x, const int* lens, int B, int frames, int channels, hipStream_t s) {
    DSH_REQUIRE(x && lens && B > 0 && frames > 0 && channels > 0, "zero_padded_frames: invalid argument");
    const size_t n = (size_t)B * frames * channels;
    hipLaunchKernelGGL(zero_padded_frames_kernel, dim3(grid_for(n)), dim3(256), 0, s, x, lens, n, frames, channels);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- window hand-off of live chains on a slot table tails[S, L, C] (fp32): row r of a window batch belongs to slot slot_idx[r] ----
// (the host refuses an index outside [0, S) and a length outside [L, T] before the launch; the kernels skip such a row all the same,
//  so that no address outside the table or the window is ever formed)
// gt[r, :L] = tails[slot_idx[r]], gt[r, L:] = 0; mask[r, :L] = 1, mask[r, L:] = 0: the inpaint dictionary of a chained window
__global__ void chain_handoff_kernel(const float* __restrict__ tails, const int* __restrict__ slot_idx, int S, size_t n, int T, int L, int C,
                                     float* __restrict__ gt, uint8_t* __restrict__ mask) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, row_n = (size_t)T * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const size_t r = i / row_n, in_row = i - r * row_n;
        const int t = (int)(in_row / C), c = (int)(in_row - (size_t)t * C);
        const int slot = slot_idx[r];
        const bool head = t < L;
        float g = 0.f;
        if (head && slot >= 0 && slot < S) g = tails[((size_t)slot * L + t) * C + c];
        gt[i] = g;
        mask[i] = head ? 1 : 0;
    }
}
int launch_chain_handoff(const float* tails, int S, const int* slot_idx, int R, int T, int L, int C, float* gt, uint8_t* mask, hipStream_t s) {
    DSH_REQUIRE(R >= 0 && S > 0 && C > 0, "chain_handoff: invalid argument");
    DSH_REQUIRE(L >= 1 && L < T, "chain_handoff: needs 1 <= overlap_len < frames");
    if (R == 0) return 0;
    DSH_REQUIRE(tails && slot_idx && gt && mask, "chain_handoff: null pointer");
    const size_t n = (size_t)R * T * C;
    hipLaunchKernelGGL(chain_handoff_kernel, dim3(grid_for(n)), dim3(256), 0, s, tails, slot_idx, S, n, T, L, C, gt, mask);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}
// tails[slot_idx[r]] = x[r, n_r - L : n_r], n_r = lens[r] (ragged batch) or T
__global__ void chain_save_tail_kernel(const float* __restrict__ x, const int* __restrict__ lens, const int* __restrict__ slot_idx, int S, size_t n,
                                       int T, int L, int C, float* __restrict__ tails) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, row_n = (size_t)L * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const size_t r = i / row_n, in_row = i - r * row_n;
        const int slot = slot_idx[r];
        const int nr = lens ? lens[r] : T;
        if (slot < 0 || slot >= S || nr < L || nr > T) continue;
        tails[(size_t)slot * row_n + in_row] = x[(r * T + (size_t)(nr - L)) * C + in_row];
    }
}
int launch_chain_save_tail(const float* x, const int* lens, const int* slot_idx, int S, int R, int T, int L, int C, float* tails, hipStream_t s) {
    DSH_REQUIRE(R >= 0 && S > 0 && C > 0, "chain_save_tail: invalid argument");
    DSH_REQUIRE(L >= 1 && L < T, "chain_save_tail: needs 1 <= overlap_len < frames");
    if (R == 0) return 0;
    DSH_REQUIRE(x && slot_idx && tails, "chain_save_tail: null pointer");
    const size_t n = (size_t)R * L * C;
    hipLaunchKernelGGL(chain_save_tail_kernel, dim3(grid_for(n)), dim3(256), 0, s, x, lens, slot_idx, S, n, T, L, C, tails);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- synchronised window batches: every window of a stream is one row of x [B, T, C]; row b's first L frames are the
// stream frames its left neighbour p = left[b] holds as its last L valid frames.  Both copies take the addBlend cross-fade of the two:
//   a = x[p, n_p - L + j, c], r = x[b, j, c], w = linspace(0, 1, L)[j]:  both <- a (1 - w) + r w      (n_p = lens[p], or T)
// The thread that owns (b, j, c) reads both elements and writes both; under the conditions check_window_sync() states no other thread
// touches either.  The host validates its copy of left / lens; a row whose DEVICE index or length is out of range is skipped all the same,
// so no address outside x is formed even if the two copies disagree.
int check_window_sync(const int32_t* left, const int32_t* lens, int B, int T, int L, std::string& err) {
#define SYNC_REQUIRE(cond, msg) do { if (!(cond)) { err = std::string("window_sync: ") + (msg); return -1; } } while (0)
    SYNC_REQUIRE(B > 0 && T > 0 && left, "invalid argument");
    SYNC_REQUIRE(L >= 1, "needs overlap_len >= 1");
    std::vector<char> is_left(B, 0);
    for (int b = 0; b < B; ++b) {
        const int p = left[b];
        if (p == -1) continue;
        SYNC_REQUIRE(p >= 0 && p < B, "a left neighbour outside the batch (-1: none)");
        SYNC_REQUIRE(p != b, "a row is its own left neighbour");
        SYNC_REQUIRE(!is_left[p], "a row is the left neighbour of two rows");
        is_left[p] = 1;
    }
    for (int b = 0; b < B; ++b) {
        const bool has_left = left[b] >= 0;
        if (!has_left && !is_left[b]) continue;
        const int n = lens ? lens[b] : T;
        SYNC_REQUIRE(n <= T, "a row length beyond the frame count");
        SYNC_REQUIRE(n >= L, "a row that shares frames is shorter than overlap_len");
        SYNC_REQUIRE(!(has_left && is_left[b]) || n >= 2 * (int64_t)L, "a row that shares frames at both ends is shorter than 2 * overlap_len");
    }
    return 0;
#undef SYNC_REQUIRE
}
__global__ void window_sync_kernel(float* __restrict__ x, const int* __restrict__ left, const int* __restrict__ lens, int B, size_t n, int T,
                                   int L, int C, int c_lo, int c_hi) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, lc = (size_t)L * C;
    const bool ranged = c_hi > c_lo;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const size_t b = i / lc, in_row = i - b * lc;
        const int j = (int)(in_row / C), c = (int)(in_row - (size_t)j * C);
        if (ranged && (c < c_lo || c >= c_hi)) continue;
        const int p = left[b];
        if (p < 0 || p >= B || (size_t)p == b) continue;
        const int np = lens ? lens[p] : T, nb = lens ? lens[b] : T;
        if (np < L || np > T || nb < L || nb > T) continue;
        const size_t ia = ((size_t)p * T + (size_t)(np - L + j)) * C + c, ir = (b * T + (size_t)j) * C + c;
        const float a = x[ia], r = x[ir];
        const float w = linspace01(L, j);
        const float v = rn_add(rn_mul(a, rn_sub(1.0f, w)), rn_mul(r, w));
        x[ia] = v;
        x[ir] = v;
    }
}
int launch_window_sync(float* x, int B, int frames, int channels, const int* left_dev, const int* lens_dev, int L, int c_lo, int c_hi,
                       hipStream_t s) {
    DSH_REQUIRE(x && left_dev && B > 0 && frames > 0 && channels > 0, "window_sync: invalid argument");
    // (L > frames: no row can share frames — the host check has refused any that would, the kernel skips every row)
    DSH_REQUIRE(L >= 1, "window_sync: needs overlap_len >= 1");
    DSH_REQUIRE(c_lo >= 0 && c_hi <= channels, "window_sync: channel range outside [0, channels]");
    const size_t n = (size_t)B * L * channels;
    hipLaunchKernelGGL(window_sync_kernel, dim3(grid_for(n)), dim3(256), 0, s, x, left_dev, lens_dev, B, n, frames, L, channels, c_lo, c_hi);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace dsh
