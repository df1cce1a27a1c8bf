// Audio front on the device (audio_front.hip): the mel spectrogram the reference's test_custom_aud computes with librosa
// (trainers/ddpm_show_trainer.py:944-1100: melspectrogram(y, sr=18000, hop_length=1200, n_mels=128)[..., :-1], power 2, no logarithm),
// a polyphase FIR resampler for caller-supplied taps, and the softmax multi-head attention core of a speech encoder.
#pragma once
#include <vector>

#include "dsh_common.h"

namespace dsh {

// One handle = one (sr, n_fft, hop, n_mels) and one stream.  The tables are built on the host in fp64 and stored as fp32; nothing touches a
// device before the first compute().
//   dft  [2 (n_fft/2 + 1), n_fft]: row k < n_fft/2 + 1 = hann[i] cos(2 pi k i / n_fft), row n_fft/2 + 1 + k = hann[i] sin(2 pi k i / n_fft)
//        (periodic Hann 0.5 - 0.5 cos(2 pi i / n_fft) folded in; the angle is reduced as (k i) mod n_fft before the fp64 cos / sin)
//   fb   [n_mels, n_fft/2 + 1]: Slaney filters from 0 to sr / 2 (see mel_tables below)
class MelFront {
public:
    MelFront(int sr, int n_fft, int hop, int n_mels, hipStream_t s);
    ~MelFront();
    int bins() const { return n_fft_ / 2 + 1; }
    int n_fft() const { return n_fft_; }
    int n_mels() const { return n_mels_; }
    int sample_rate() const { return sr_; }
    const std::vector<float>& dft() const { return dft_; }
    const std::vector<float>& fb() const { return fb_; }
    // frames of a signal of `len` samples: len / hop (the reference drops the last of the 1 + len / hop centred frames); -1 when the reflect
    // padding (len >= n_fft / 2 + 1) or len >= hop does not hold
    long long num_frames(long long len) const;
    int compute(const float* wave, int B, long long len, float* mel);
    // rows padded to `len` samples, row b owning lens[b] of them (DEVICE int32, each with num_frames(lens[b]) >= 1 and <= len: the caller's
    // check): mel [B, num_frames(len), n_mels], row b bit for bit compute() on its own lens[b] samples, 0 behind its lens[b] / hop frames.
    // No sample behind lens[b] is read.
    int compute_ragged(const float* wave, int B, long long len, const int* lens, float* mel);
private:
    int run(const char* what, const float* wave, int B, long long len, const int* lens, float* mel);
    int upload();
    int reserve(int B, long long len);
    void release_buffers();
    int sr_, n_fft_, hop_, n_mels_;
    int Nd_ = 0, Kf_ = 0;            // DFT columns (2 bins) rounded up to 4; spectrum width (bins) rounded up to the 32-float K tile
    hipStream_t stream_;
    bool owns_stream_ = false, uploaded_ = false;
    std::vector<float> dft_, fb_;
    float *dft_dev_ = nullptr, *fb_dev_ = nullptr, *zero_dev_ = nullptr;
    float *pad_ = nullptr, *spec_ = nullptr, *pow_ = nullptr;
    long long cap_pad_ = 0, cap_rows_ = 0;
};

// y[b, j] = sum_k taps[k] x[b, (j down + (n_taps - 1) / 2 - k) / up] over the taps k for which the index is an integer inside [0, n), k
// ascending: scipy.signal.resample_poly's zero-stuff / filter / decimate with the taps centred, n_out = ceil(n up / down) samples per row.
// taps is a DEVICE array of n_taps (odd) floats.
long long resample_poly_len(long long n, int up, int down);
int launch_resample_poly(const float* x, int B, long long n, int up, int down, const float* taps, int n_taps, float* y, hipStream_t s);
// x [B, n] of which row b owns lens[b] samples (DEVICE int32, clamped to [0, n]; nullptr: every row owns n): y [B, resample_poly_len(n)], row b
// what the dense call gives for its own samples alone, 0 behind resample_poly_len(lens[b]).  No sample behind lens[b] is read.
int launch_resample_poly_ragged(const float* x, int B, long long n, const int* lens, int up, int down, const float* taps, int n_taps, float* y,
                                hipStream_t s);

// softmax multi-head attention core, 64-wide heads, no mask: qkv [B, M, 3 H 64] = (q | k | v), q already scaled;
// out[b, t, h 64 + d] = sum_s softmax_s(q[b, t, h] . k[b, s, h]) v[b, s, h 64 + d]
int launch_softmax_attention(const float* qkv, int B, int M, int H, float* out, hipStream_t s);
// the same for rows of M_max frames of which row b owns lens[b] (DEVICE int32, clamped to [0, M_max]): keys and queries < lens[b] only, the bits
// of the dense call on the row alone at M = lens[b]; out[b, t >= lens[b]] = 0; no frame >= lens[b] is read
int launch_softmax_attention_ragged(const float* qkv, int B, int M_max, int H, const int* lens, float* out, hipStream_t s);
// both on bf16 operands (v_mfma_f32_32x32x16_bf16): bf16 q^ | k^ | v in, fp32 logits and online softmax, the second product's operand is
// RNE_bf16(exp(s - m)) while the row sum adds the unrounded values, o = (sum p^ v) / l stored RNE bf16.  Same contracts as the fp32 pair.
int launch_softmax_attention_bf16(const bf16* qkv, int B, int M, int H, bf16* out, hipStream_t s);
int launch_softmax_attention_bf16_ragged(const bf16* qkv, int B, int M_max, int H, const int* lens, bf16* out, hipStream_t s);

}  // namespace dsh
