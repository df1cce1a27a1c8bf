// Audio front on the device: mel spectrogram, polyphase resampler, softmax attention core.  fp32 throughout, every matrix product on the
// exact-fp32 matrix pipe (v_mfma_f32_32x32x2_f32), except the last section: the attention core once more on bf16 operands for the HuBERT
// encoder's bf16 precision mode.  Every reduction has a fixed order (no atomics): two runs give identical bits, and the result of batch row b
// does not depend on the batch size.
//
// Mel spectrogram (MelFront::compute), four launches:
//   1. reflect_pad_kernel      wave [B, len] -> pad [B, Lp], Lp = len + n_fft rounded up to 4 floats: pad[i] = wave[reflect(i - n_fft / 2)]
//   2. conv_gemm_f32_kernel    the windowed DFT as the implicit GEMM of pose_encoder.hip: frame j of clip b is the CONTIGUOUS slice
//                              pad[b, hop j : hop j + n_fft], so A row base = b Lp + j hop (overlapping rows), K = n_fft, W = the
//                              window-folded (cos | sin) table [2 bins (+ pad to 4), n_fft] -> spec [B N, Nd]
//   3. power_rows_kernel       pow[m, k] = re^2 + im^2 for k < bins, 0 on the K pad up to the 32-float tile
//   4. conv_gemm_f32_kernel    the filterbank: pow [B N, Kf] x fb [n_mels, Kf]^T -> mel [B, N, n_mels]
// A silent input gives exact zeros: every product is 0 x table and the bias added in the GEMM epilogue is +0.
// The power pass is a row pass: fusing it into the DFT's epilogue needs the cos and the sin column of a bin in the same lane, i.e. a table with
// the two interleaved in groups of four columns; not measured against the row pass yet.
#include <cmath>
#include <cstring>

#include "audio_front.h"
#include "fgd.h"

namespace dsh {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- host tables (fp64 -> fp32) ---------------------------------------------------------------------------------------------------
static double hz_to_mel(double f) {
    // Slaney: linear below 1000 Hz (200 / 3 Hz per mel), logarithmic above (27 mels per factor 6.4)
    return f < 1000.0 ? 3.0 * f / 200.0 : 15.0 + 27.0 * std::log(f / 1000.0) / std::log(6.4);
}
static double mel_to_hz(double m) { return m < 15.0 ? 200.0 * m / 3.0 : 1000.0 * std::exp(std::log(6.4) * (m - 15.0) / 27.0); }

MelFront::MelFront(int sr, int n_fft, int hop, int n_mels, hipStream_t s) : sr_(sr), n_fft_(n_fft), hop_(hop), n_mels_(n_mels), stream_(s) {
    const int nb = bins();
    Nd_ = round_up(2 * nb, 4);
    Kf_ = round_up(nb, 32);
    dft_.assign((size_t)2 * nb * n_fft, 0.0f);
    std::vector<double> win(n_fft), cs(n_fft), sn(n_fft);
    for (int i = 0; i < n_fft; ++i) {
        const double a = 2.0 * M_PI * (double)i / (double)n_fft;
        win[i] = 0.5 - 0.5 * std::cos(a);
        cs[i] = std::cos(a);
        sn[i] = std::sin(a);
    }
    for (int k = 0; k < nb; ++k)
        for (int i = 0; i < n_fft; ++i) {
            const int r = (int)(((long long)k * i) % n_fft);        // exact reduction of the angle
            dft_[(size_t)k * n_fft + i] = (float)(win[i] * cs[r]);
            dft_[(size_t)(nb + k) * n_fft + i] = (float)(win[i] * sn[r]);
        }
    fb_.assign((size_t)n_mels * nb, 0.0f);
    std::vector<double> pts(n_mels + 2);
    const double m_lo = hz_to_mel(0.0), m_hi = hz_to_mel(0.5 * sr);
    for (int i = 0; i < n_mels + 2; ++i) pts[i] = mel_to_hz(m_lo + (m_hi - m_lo) * (double)i / (double)(n_mels + 1));
    for (int i = 0; i < n_mels; ++i)
        for (int k = 0; k < nb; ++k) {
            const double f = (double)k * (double)sr / (double)n_fft;
            const double lo = (f - pts[i]) / (pts[i + 1] - pts[i]), up = (pts[i + 2] - f) / (pts[i + 2] - pts[i + 1]);
            const double tri = std::fmax(0.0, std::fmin(lo, up));
            fb_[(size_t)i * nb + k] = (float)(tri * (2.0 / (pts[i + 2] - pts[i])));
        }
}

void MelFront::release_buffers() {
    for (float** p : {&pad_, &spec_, &pow_}) { if (*p) (void)hipFree(*p); *p = nullptr; }
    cap_pad_ = cap_rows_ = 0;
}

MelFront::~MelFront() {
    if (stream_ && uploaded_) (void)hipStreamSynchronize(stream_);
    release_buffers();
    for (float* p : {dft_dev_, fb_dev_, zero_dev_}) if (p) (void)hipFree(p);
    if (owns_stream_) (void)hipStreamDestroy(stream_);
}

long long MelFront::num_frames(long long len) const {
    if (len < n_fft_ / 2 + 1 || len < hop_) return -1;
    return len / hop_;
}

int MelFront::upload() {
    if (uploaded_) return 0;
    int ndev = 0;
    DSH_HIP_CHECK(hipGetDeviceCount(&ndev));
    DSH_REQUIRE(ndev > 0, "no HIP device visible: this library has no CPU fallback");
    if (stream_ == nullptr) {
        DSH_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamDefault));
        owns_stream_ = true;
    }
    const int nb = bins();
    // device copies: the DFT table with its rows padded to Nd_ (zero rows: their spectrum columns are 0 and never read), the filterbank with
    // its K padded to the 32-float tile
    std::vector<float> d((size_t)Nd_ * n_fft_, 0.0f), f((size_t)n_mels_ * Kf_, 0.0f);
    memcpy(d.data(), dft_.data(), dft_.size() * sizeof(float));
    for (int i = 0; i < n_mels_; ++i) memcpy(&f[(size_t)i * Kf_], &fb_[(size_t)i * nb], nb * sizeof(float));
    const size_t nz = (size_t)(Nd_ > n_mels_ ? Nd_ : n_mels_);
    DSH_HIP_CHECK(hipMalloc((void**)&dft_dev_, d.size() * sizeof(float)));
    DSH_HIP_CHECK(hipMalloc((void**)&fb_dev_, f.size() * sizeof(float)));
    DSH_HIP_CHECK(hipMalloc((void**)&zero_dev_, nz * sizeof(float)));
    DSH_HIP_CHECK(hipMemcpy(dft_dev_, d.data(), d.size() * sizeof(float), hipMemcpyHostToDevice));
    DSH_HIP_CHECK(hipMemcpy(fb_dev_, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
    DSH_HIP_CHECK(hipMemset(zero_dev_, 0, nz * sizeof(float)));
    uploaded_ = true;
    return 0;
}

int MelFront::reserve(int B, long long len) {
    const long long Lp = (len + n_fft_ + 3) / 4 * 4, rows = (long long)B * (len / hop_);
    if ((long long)B * Lp <= cap_pad_ && rows <= cap_rows_) return 0;
    DSH_HIP_CHECK(hipStreamSynchronize(stream_));          // (growing waits for launches that still use the old buffers)
    release_buffers();
    DSH_HIP_CHECK(hipMalloc((void**)&pad_, (size_t)B * Lp * sizeof(float)));
    DSH_HIP_CHECK(hipMalloc((void**)&spec_, (size_t)rows * Nd_ * sizeof(float)));
    DSH_HIP_CHECK(hipMalloc((void**)&pow_, (size_t)rows * Kf_ * sizeof(float)));
    cap_pad_ = (long long)B * Lp;
    cap_rows_ = rows;
    return 0;
}

// lens (nullable): row b of x [B, ld] holds lens[b] samples of its own; the reflection is about ITS last sample and everything behind
// lens[b] + n_fft is 0, so no sample >= lens[b] is read.  A count outside [half + 1, ld] (the callers refuse it on the host) gives a zero row.
__global__ void reflect_pad_kernel(const float* __restrict__ x, long long ld, const int* __restrict__ lens, float* __restrict__ y, long long Lp,
                                   int half, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long b = (long long)(i / (size_t)Lp), c = (long long)(i % (size_t)Lp);
    long long len = ld;
    if (lens) {
        len = lens[b];
        if (len < half + 1 || len > ld) len = -2 * (long long)half;      // (c < len + 2 half never holds)
    }
    float v = 0.0f;                                         // (columns behind len + n_fft: the pad to 4 floats)
    if (c < len + 2 * half) {
        long long j = c - half;
        if (j < 0) j = -j;                                  // len >= half + 1: one reflection is enough on either side
        else if (j >= len) j = 2 * (len - 1) - j;
        v = x[b * ld + j];
    }
    y[i] = v;
}

// y [B, N, C]: frames t >= lens[b] / div of batch row b become 0 (C % 4 == 0)
__global__ void zero_tail_frames_kernel(float* __restrict__ y, long long N, int C4, const int* __restrict__ lens, int div, size_t n4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const size_t row = i / (size_t)C4;
    const long long b = (long long)(row / (size_t)N), t = (long long)(row % (size_t)N);
    const int own = lens[b] < 0 ? 0 : lens[b] / div;
    if (t >= own) reinterpret_cast<f32x4*>(y)[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

__global__ void power_rows_kernel(const float* __restrict__ spec, int Nd, int nb, float* __restrict__ pw, int Kf, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t m = i / (size_t)Kf;
    const int k = (int)(i % (size_t)Kf);
    float v = 0.0f;
    if (k < nb) {
        const float re = spec[m * Nd + k], im = spec[m * Nd + nb + k];
        v = re * re + im * im;
    }
    pw[i] = v;
}

int MelFront::compute(const float* wave, int B, long long len, float* mel) { return run("dsh_mel_compute", wave, B, len, nullptr, mel); }

// Rows of `len` samples of which row b owns lens[b] (DEVICE int32; the host-side callers have checked num_frames(lens[b]) >= 1 and
// lens[b] <= len).  Only the padding knows the row's own length: frame j < lens[b] / hop of the padded row is the slice the dense call at
// len = lens[b] forms, the two GEMMs give every output element one accumulator with K ascending wherever the row sits in M, so mel[b, j] has the
// bits of compute() on row b alone.  The frames behind are finite (the pad row is zeros there) and are overwritten with 0.
int MelFront::compute_ragged(const float* wave, int B, long long len, const int* lens, float* mel) {
    DSH_REQUIRE(lens, "dsh_mel_compute_ragged: null lengths");
    DSH_REQUIRE(len < (1ll << 31), "dsh_mel_compute_ragged: rows of at most 2^31 - 1 samples");
    return run("dsh_mel_compute_ragged", wave, B, len, lens, mel);
}

int MelFront::run(const char* what, const float* wave, int B, long long len, const int* lens, float* mel) {
    DSH_REQUIRE(wave && mel, std::string(what) + ": null tensor");
    DSH_REQUIRE(B >= 1, std::string(what) + ": batch must be positive");
    const long long N = num_frames(len);
    if (N < 1) {
        set_last_error("invalid argument: " + std::string(what) + ": " + std::to_string(len) + " samples; the reflect padding needs " +
                       std::to_string(n_fft_ / 2 + 1) + " and one frame " + std::to_string(hop_));
        return -1;
    }
    const long long Lp = (len + n_fft_ + 3) / 4 * 4;
    DSH_REQUIRE((long long)B * N < (1ll << 31) / 64 && (long long)B * Lp < (1ll << 40), std::string(what) + ": batch too large");
    // the last frame read ends at hop (N - 1) + n_fft <= len - hop + n_fft < len + n_fft <= Lp: inside the padded row
    if (int e = upload()) return e;
    if (int e = reserve(B, len)) return e;
    const int M = (int)((long long)B * N);
    {
        const size_t n = (size_t)B * Lp;
        hipLaunchKernelGGL(reflect_pad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream_, wave, len, lens, pad_, Lp, n_fft_ / 2, n);
        DSH_HIP_CHECK(hipGetLastError());
    }
    {
        ConvGemmArgs a{};
        a.X = pad_; a.x_clip = Lp; a.x_step = hop_;
        a.W = dft_dev_; a.ldw = n_fft_; a.bias = zero_dev_;
        a.Y = spec_; a.y_clip = N * Nd_;
        a.Tout = (int)N; a.M = M; a.N = Nd_; a.Kreal = n_fft_; a.Kp = n_fft_;
        if (int e = launch_conv_gemm_f32(a, stream_)) return e;
    }
    {
        const size_t n = (size_t)M * Kf_;
        hipLaunchKernelGGL(power_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream_, spec_, Nd_, bins(), pow_, Kf_, n);
        DSH_HIP_CHECK(hipGetLastError());
    }
    {
        ConvGemmArgs a{};
        a.X = pow_; a.x_clip = N * Kf_; a.x_step = Kf_;
        a.W = fb_dev_; a.ldw = Kf_; a.bias = zero_dev_;
        a.Y = mel; a.y_clip = N * n_mels_;
        a.Tout = (int)N; a.M = M; a.N = n_mels_; a.Kreal = Kf_; a.Kp = Kf_;
        if (int e = launch_conv_gemm_f32(a, stream_)) return e;
    }
    if (lens) {
        const size_t n4 = (size_t)M * (n_mels_ / 4);
        hipLaunchKernelGGL(zero_tail_frames_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream_, mel, N, n_mels_ / 4, lens, hop_, n4);
        DSH_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

// ---- polyphase FIR resampler -------------------------------------------------------------------------------------------------------
long long resample_poly_len(long long n, int up, int down) { return (n * up + down - 1) / down; }

// One lane per output sample.  Output j sits at position m = j down + half of the zero-stuffed signal convolved with the taps; only the taps
// k = m (mod up) meet a non-zero sample x[(m - k) / up]: about n_taps / up products, added in ascending tap order.
// lens (nullable): row b of x [B, ld] holds lens[b] samples of its own (clamped to [0, ld]); the taps see nothing behind them and the outputs
// behind ceil(lens[b] up / down) are 0.
__global__ void resample_poly_kernel(const float* __restrict__ x, long long ld, const int* __restrict__ lens, int up, int down,
                                     const float* __restrict__ taps, int n_taps, float* __restrict__ y, long long n_out, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long b = (long long)(i / (size_t)n_out), j = (long long)(i % (size_t)n_out);
    long long n = ld;
    if (lens) {
        n = lens[b];
        n = n < 0 ? 0 : (n > ld ? ld : n);
        if (j >= (n * up + down - 1) / down) { y[i] = 0.0f; return; }
    }
    const long long m = j * down + (n_taps - 1) / 2;
    long long k = m % up;
    const long long k_min = m - (n - 1) * up;              // x index (m - k) / up <= n - 1
    if (k < k_min) k += (k_min - k + up - 1) / up * up;
    const float* xr = x + b * ld;
    float acc = 0.0f;
    for (; k < n_taps && k <= m; k += up) acc = fmaf(taps[k], xr[(m - k) / up], acc);
    y[i] = acc;
}

int launch_resample_poly(const float* x, int B, long long n, int up, int down, const float* taps, int n_taps, float* y, hipStream_t s) {
    return launch_resample_poly_ragged(x, B, n, nullptr, up, down, taps, n_taps, y, s);
}

int launch_resample_poly_ragged(const float* x, int B, long long n, const int* lens, int up, int down, const float* taps, int n_taps, float* y,
                                hipStream_t s) {
    DSH_REQUIRE(x && taps && y, "resample_poly: null pointer");
    DSH_REQUIRE(!lens || n < (1ll << 31), "resample_poly: ragged rows of at most 2^31 - 1 samples");
    DSH_REQUIRE(B >= 1 && n >= 1, "resample_poly: batch and length must be positive");
    DSH_REQUIRE(up >= 1 && down >= 1 && n_taps >= 1 && n_taps % 2 == 1, "resample_poly: up, down >= 1 and an odd number of taps");
    DSH_REQUIRE(n < (1ll << 40) / up && n < (1ll << 40) / down, "resample_poly: signal too long");
    const long long n_out = resample_poly_len(n, up, down);
    const size_t total = (size_t)B * n_out;
    DSH_REQUIRE(total < ((size_t)1 << 31) * 256, "resample_poly: batch too large");
    hipLaunchKernelGGL(resample_poly_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, n, lens, up, down, taps, n_taps, y, n_out, total);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- softmax attention ----------------------------------------------------------------------------------------------------------------
// One wave per (batch row, head, tile of 32 queries); keys in tiles of 32, online max / sum (the running maximum carries logits of any size).
// Both products run on the 32x32x2 fp32 MFMA without LDS and without moving data between lanes:
//   S^T = K Q^T   A operand = the key tile (row i = key), B operand = the queries (column j = query).  Lane l holds the 32 channels
//                 32 (l >> 5) .. + 32 of its key and of its query; MFMA step s multiplies channel 32 (l >> 5) + s of both, i.e. the k slots
//                 are permuted identically on both sides, which leaves the dot product unchanged.  The result has the QUERY on the lane
//                 (j = l & 31) and 16 keys in the registers (key i = (r & 3) + 8 (r >> 2) + 4 (l >> 5)): the softmax statistics of a query
//                 are 16 registers of one lane and one exchange with lane l ^ 32.
//   O^T = V^T P^T sums over the ROW index of S^T, so register r of S^T is directly the B operand of step r (k slot (l >> 5) = key
//                 (r & 3) + 8 (r >> 2) + 4 (l >> 5)); the A operand of that step is V[that key][channel l & 31 (+ 32)].  O^T again has
//                 the query on the lane, so the rescaling by exp(m_old - m_new) and the final 1 / sum are per-lane scalars.
// Keys >= M of the last tile get the logit -inf: their weight is exp(-inf) = 0 exactly; their K / V rows are loaded from row M - 1.
// RAGGED: batch row b has lens[b] (clamped to [0, M_max]) frames of its own inside a row of M_max; the body below runs with M = lens[b] and
// only the row base and the output row use M_max, so it issues the loads, MFMAs and exponentials of the dense kernel at M = lens[b] in
// the same order: the row has the same bits.  A frame >= lens[b] is never loaded (a NaN there would survive a zero weight); query tiles that
// start behind lens[b] leave at the top; output frames lens[b] .. M_max - 1 are written as 0.
__device__ __forceinline__ void attention_zero_row(float* orow, int half) {
    const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        *reinterpret_cast<f32x4*>(orow + 8 * g + 4 * half) = z;
        *reinterpret_cast<f32x4*>(orow + 32 + 8 * g + 4 * half) = z;
    }
}

template <bool RAGGED>
__global__ __launch_bounds__(64) void softmax_attention_f32_kernel(const float* __restrict__ qkv, int M_max, int H, const int* __restrict__ lens,
                                                                  float* __restrict__ out, int q_tiles) {
    const int lane = threadIdx.x, half = lane >> 5, col = lane & 31;
    const int qt = blockIdx.x % q_tiles, bh = blockIdx.x / q_tiles, h = bh % H, b = bh / H;
    const size_t ld = (size_t)3 * H * 64;
    int M = M_max;
    if (RAGGED) {
        M = lens[b];
        M = M < 0 ? 0 : (M > M_max ? M_max : M);
        if (qt * 32 >= M) {                                 // (uniform over the wave) nothing of this tile is a frame of the row
            if (qt * 32 + col < M_max) attention_zero_row(out + ((size_t)b * M_max + qt * 32 + col) * ((size_t)H * 64) + (size_t)h * 64, half);
            return;
        }
    }
    const float* base = qkv + (size_t)b * M_max * ld + (size_t)h * 64;
    const float* kbase = base + (size_t)H * 64;
    const float* vbase = base + (size_t)2 * H * 64;
    const int q_row = qt * 32 + col;
    const int q_ld = q_row < M ? q_row : M - 1;

    float q[32];
    {
        const f32x4* src = reinterpret_cast<const f32x4*>(base + (size_t)q_ld * ld + half * 32);
#pragma unroll
        for (int i = 0; i < 8; ++i) { const f32x4 t = src[i]; q[4 * i] = t.x; q[4 * i + 1] = t.y; q[4 * i + 2] = t.z; q[4 * i + 3] = t.w; }
    }
    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.0f; o1[r] = 0.0f; }
    float m_run = -INFINITY, l_run = 0.0f;

    for (int k0 = 0; k0 < M; k0 += 32) {
        float kk[32];
        {
            const int kr = k0 + col < M ? k0 + col : M - 1;
            const f32x4* src = reinterpret_cast<const f32x4*>(kbase + (size_t)kr * ld + half * 32);
#pragma unroll
            for (int i = 0; i < 8; ++i) { const f32x4 t = src[i]; kk[4 * i] = t.x; kk[4 * i + 1] = t.y; kk[4 * i + 2] = t.z; kk[4 * i + 3] = t.w; }
        }
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.0f;
#pragma unroll
        for (int c = 0; c < 32; ++c) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kk[c], q[c], s, 0, 0, 0);
        float mt = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            s[r] = key < M ? s[r] : -INFINITY;
            mt = fmaxf(mt, s[r]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float m_new = fmaxf(m_run, mt);               // finite: key k0 is valid in every tile
        const float alpha = expf(m_run - m_new);            // first tile: exp(-inf) = 0
        float psum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = expf(s[r] - m_new); psum += s[r]; }
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            key = key < M ? key : M - 1;
            const float* vr = vbase + (size_t)key * ld + col;
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[0], s[r], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[32], s[r], o1, 0, 0, 0);
        }
    }
    const float inv = 1.0f / (l_run + __shfl_xor(l_run, 32));
    float* orow = out + ((size_t)b * M_max + q_row) * ((size_t)H * 64) + (size_t)h * 64;
    if (q_row >= M) {
        if (RAGGED && q_row < M_max) attention_zero_row(orow, half);
        return;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f32x4 a, c;
        a.x = o0[4 * g] * inv; a.y = o0[4 * g + 1] * inv; a.z = o0[4 * g + 2] * inv; a.w = o0[4 * g + 3] * inv;
        c.x = o1[4 * g] * inv; c.y = o1[4 * g + 1] * inv; c.z = o1[4 * g + 2] * inv; c.w = o1[4 * g + 3] * inv;
        *reinterpret_cast<f32x4*>(orow + 8 * g + 4 * half) = a;
        *reinterpret_cast<f32x4*>(orow + 32 + 8 * g + 4 * half) = c;
    }
}

int launch_softmax_attention(const float* qkv, int B, int M, int H, float* out, hipStream_t s) {
    DSH_REQUIRE(qkv && out, "softmax attention: null pointer");
    DSH_REQUIRE(B >= 1 && M >= 1 && H >= 1, "softmax attention: B, M and H must be positive");
    DSH_REQUIRE(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)out % 16) == 0, "softmax attention: operands must be 16-byte aligned");
    const int q_tiles = ceil_div(M, 32);
    DSH_REQUIRE((long long)B * H * q_tiles < (1ll << 31), "softmax attention: batch too large");
    hipLaunchKernelGGL(softmax_attention_f32_kernel<false>, dim3((unsigned)(B * H * q_tiles)), dim3(64), 0, s, qkv, M, H, (const int*)nullptr, out, q_tiles);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_softmax_attention_ragged(const float* qkv, int B, int M_max, int H, const int* lens, float* out, hipStream_t s) {
    DSH_REQUIRE(qkv && out && lens, "softmax attention (ragged): null pointer");
    DSH_REQUIRE(B >= 1 && M_max >= 1 && H >= 1, "softmax attention (ragged): B, M_max and H must be positive");
    DSH_REQUIRE(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)out % 16) == 0, "softmax attention (ragged): operands must be 16-byte aligned");
    const int q_tiles = ceil_div(M_max, 32);
    DSH_REQUIRE((long long)B * H * q_tiles < (1ll << 31), "softmax attention (ragged): batch too large");
    hipLaunchKernelGGL(softmax_attention_f32_kernel<true>, dim3((unsigned)(B * H * q_tiles)), dim3(64), 0, s, qkv, M_max, H, lens, out, q_tiles);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- softmax attention on bf16 operands -------------------------------------------------------------------------------------------------
// The kernel above on v_mfma_f32_32x32x16_bf16: bf16 q^ | k^ | v in, bf16 out, the same wave per (batch row, head, 32 queries), the same
// orientation, the same online max / sum in fp32 (no deferred rescaling).
//   S^T = K Q^T   four MFMAs over the 64 channels: element j of lane (c, half) of step s is channel 16 s + 8 half + j of key c (A) and of
//                 query c (B), one 16-byte load each.  fp32 logits, the query on the lane.
//   p = exp(s - m) in fp32; the row sum l adds these UNROUNDED values; the operand of the second product is RNE_bf16(p).
//   O^T = V^T P^T registers 8 t .. 8 t + 7 of S^T, packed to bf16, are the B fragment of step t (t = 0, 1) as they stand: element j is key
//                 16 t + 8 (j >> 2) + 4 half + (j & 3), and the A fragment takes V of that same key.  Lane c loads channels (2 c, 2 c + 1) of
//                 the key as one dword: the low halves feed the accumulator of the even channels (row i = channel 2 i), the high halves that of
//                 the odd ones, so a lane ends up with eight CONSECUTIVE channels 16 g + 8 half .. + 7 per register group g: one 16-byte store.
//   o = (sum p^ v) / l in fp32, RNE bf16 store.
// Keys >= M get the logit -inf and the weight exactly 0; their rows are never loaded (the loads clamp to row M - 1).  RAGGED as above.
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void attention_zero_row_bf16(bf16* orow, int half) {
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int g = 0; g < 4; ++g) *reinterpret_cast<u32x4*>(orow + 16 * g + 8 * half) = z;
}

template <bool RAGGED>
__global__ __launch_bounds__(64) void softmax_attention_bf16_kernel(const bf16* __restrict__ qkv, int M_max, int H, const int* __restrict__ lens,
                                                                   bf16* __restrict__ out, int q_tiles) {
    const int lane = threadIdx.x, half = lane >> 5, col = lane & 31;
    const int qt = blockIdx.x % q_tiles, bh = blockIdx.x / q_tiles, h = bh % H, b = bh / H;
    const size_t ld = (size_t)3 * H * 64;
    int M = M_max;
    if (RAGGED) {
        M = lens[b];
        M = M < 0 ? 0 : (M > M_max ? M_max : M);
        if (qt * 32 >= M) {                                 // (uniform over the wave) nothing of this tile is a frame of the row
            if (qt * 32 + col < M_max) attention_zero_row_bf16(out + ((size_t)b * M_max + qt * 32 + col) * ((size_t)H * 64) + (size_t)h * 64, half);
            return;
        }
    }
    const bf16* base = qkv + (size_t)b * M_max * ld + (size_t)h * 64;
    const bf16* kbase = base + (size_t)H * 64;
    const bf16* vbase = base + (size_t)2 * H * 64;
    const int q_row = qt * 32 + col;
    const int q_ld = q_row < M ? q_row : M - 1;

    bf16x8 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)q_ld * ld + 16 * s + 8 * half);
    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.0f; o1[r] = 0.0f; }
    float m_run = -INFINITY, l_run = 0.0f;

    for (int k0 = 0; k0 < M; k0 += 32) {
        const int kr = k0 + col < M ? k0 + col : M - 1;
        bf16x8 kf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) kf[s] = *reinterpret_cast<const bf16x8*>(kbase + (size_t)kr * ld + 16 * s + 8 * half);
        // the V dwords of this tile: issued in front of the logits, used behind the softmax
        uint32_t vw[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            key = key < M ? key : M - 1;
            vw[r] = *reinterpret_cast<const uint32_t*>(vbase + (size_t)key * ld + 2 * col);
        }
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[c], qf[c], s, 0, 0, 0);
        float mt = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            s[r] = key < M ? s[r] : -INFINITY;
            mt = fmaxf(mt, s[r]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float m_new = fmaxf(m_run, mt);               // finite: key k0 is valid in every tile
        const float alpha = expf(m_run - m_new);            // first tile: exp(-inf) = 0
        float psum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = expf(s[r] - m_new); psum += s[r]; }
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            u32x4 pf, v0, v1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t wa = vw[8 * t + 2 * j], wb = vw[8 * t + 2 * j + 1];
                pf[j] = pack_bf16_pair(s[8 * t + 2 * j], s[8 * t + 2 * j + 1]);
                v0[j] = (wa & 0xffffu) | (wb << 16);
                v1[j] = (wa >> 16) | (wb & 0xffff0000u);
            }
            o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, v0), __builtin_bit_cast(bf16x8, pf), o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, v1), __builtin_bit_cast(bf16x8, pf), o1, 0, 0, 0);
        }
    }
    const float l = l_run + __shfl_xor(l_run, 32);
    bf16* orow = out + ((size_t)b * M_max + q_row) * ((size_t)H * 64) + (size_t)h * 64;
    if (q_row >= M) {
        if (RAGGED && q_row < M_max) attention_zero_row_bf16(orow, half);
        return;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = pack_bf16_pair(o0[4 * g + e] / l, o1[4 * g + e] / l);
        *reinterpret_cast<u32x4*>(orow + 16 * g + 8 * half) = o;
    }
}

static int launch_softmax_attention_bf16_any(const char* what, const bf16* qkv, int B, int M, int H, const int* lens, bool ragged, bf16* out,
                                             hipStream_t s) {
    DSH_REQUIRE(qkv && out && (!ragged || lens), std::string(what) + ": null pointer");
    DSH_REQUIRE(B >= 1 && M >= 1 && H >= 1, std::string(what) + ": B, M and H must be positive");
    DSH_REQUIRE(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)out % 16) == 0, std::string(what) + ": operands must be 16-byte aligned");
    const int q_tiles = ceil_div(M, 32);
    DSH_REQUIRE((long long)B * H * q_tiles < (1ll << 31), std::string(what) + ": batch too large");
    if (ragged) hipLaunchKernelGGL(softmax_attention_bf16_kernel<true>, dim3((unsigned)(B * H * q_tiles)), dim3(64), 0, s, qkv, M, H, lens, out, q_tiles);
    else hipLaunchKernelGGL(softmax_attention_bf16_kernel<false>, dim3((unsigned)(B * H * q_tiles)), dim3(64), 0, s, qkv, M, H, (const int*)nullptr, out, q_tiles);
    DSH_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_softmax_attention_bf16(const bf16* qkv, int B, int M, int H, bf16* out, hipStream_t s) {
    return launch_softmax_attention_bf16_any("softmax attention (bf16)", qkv, B, M, H, nullptr, false, out, s);
}

int launch_softmax_attention_bf16_ragged(const bf16* qkv, int B, int M_max, int H, const int* lens, bf16* out, hipStream_t s) {
    return launch_softmax_attention_bf16_any("softmax attention (bf16, ragged)", qkv, B, M_max, H, lens, true, out, s);
}

}  // namespace dsh
