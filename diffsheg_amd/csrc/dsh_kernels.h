// Launcher declarations for the non-GEMM kernels (rowops.hip, attention.hip, sampler_kernels.hip).
#pragma once
#include "dsh_common.h"

namespace dsh {

// virtual concat row [h | audio_proj | hubert128 | expr_x0]  (transformer.py:304-312)
struct ConcatSegs {
    const float* p0; int ld0, w0;   // latent h, fp32
    const void* p1;  int ld1, w1;   // element type T
    const void* p2;  int ld2, w2;   // element type T
    const float* p3; int ld3, w3;   // fp32 (w3 may be 0)
};

// fp32 parity path: Linear with the LayerNorm (folded, pro 1) or StylizationBlock front (LN -> FiLM -> SiLU, pro 2) in front of it
// in one launch (gemm_f32_pro.hip).  All pointers fp32.
struct GemmProArgs {
    int pro;                            // 1: folded LayerNorm over up to four concat segments; 2: StylizationBlock front
    const float* seg[4]; int seg_ld[4]; // A rows: K tile kt (32 floats) comes from segment j with seg_end[j - 1] <= kt < seg_end[j], at column 32 (kt - seg_end[j - 1])
    int seg_end[4];                     //   (pro 2: seg[0] only)
    int k_real;                         // LayerNorm width (K - k_real trailing columns are zero padding)
    const float* W; int ldw;            // [N, K]  (pro 1: gamma folded in)
    const float* bias;                  // [N]     (pro 1: b + W beta)
    const float* fc;                    // [N]     pro 1: row sums of the folded weight
    const float* film; int film_ld, film_off, frames, bmod;   // pro 2: per-clip [scale'(K) | shift'(K)] with the LayerNorm affine folded in; clip = (row / frames) % bmod
    const float* R; int ldr;            // residual or null
    float* C; int ldc;                  // output
    int M, N, K, act;
    int nt_n, nt_m;                     // (launcher)
    // per-row group moments (mean_g, sum (x - mean_g)^2) over groups of consecutive columns, [M][groups] float2:
    const float* stats; int stat_groups, stat_gs;   // pro 2, nullable: moments of the INPUT rows left by its producer (no pass over the rows here)
    float* stats_out;                   // nullable: moments of the OUTPUT rows in groups of 32 columns ([M][N / 32] float2; N % 64 == 0)
    const float* row_const; int n_const_rows;   // epilogue: + row_const[n] on rows < n_const_rows, after the residual (the CFG-null constant of the next layer)
    int mma;                            // 0: exact fp32 MFMA (gemm_f32_pro.hip); 1: split bf16, three bf16 MFMAs per product (gemm_f32_split.hip) — W is then the
                                        //    operand PACKED by launch_split_pack_weight, same shape and row stride
    int tile;                           // mma 1: 0 the launcher picks; 1 / 2: 64 x 64 / 128 x 128 tiles (the bits do not depend on it)
    int abl;                            // ablation bits (DSH_GP_ABL, bench only; results are garbage): 1 no global loads in the loop, 2 no LDS writes, 4 no fragment reads, 8 no MFMAs, 16 no barrier
};
int launch_gemm_f32_pro(const GemmProArgs& a, hipStream_t s);
// split-bf16 form of the same launches (gemm_f32_split.hip).  The one packer of its W operand: [N][ldw] fp32 with K whole 32-float tiles -> per K
// tile [hi(32 bf16) | lo(32 bf16)], hi = RNE_bf16(w), lo = RNE_bf16(w - hi), in `out` ([N][ldw] 32-bit words).  Once per weight, never per launch.
int launch_split_pack_weight(const float* W, int N, int K, int ldw, uint32_t* out, hipStream_t s);
int launch_gemm_f32_split(const GemmProArgs& a, hipStream_t s);   // (through launch_gemm_f32_pro with a.mma = 1)

// bf16 HuBERT layers: C = act(pro(A) W^T + bias) (+ R) on the bf16 matrix pipe (gemm_bf16_pro.hip).  M >= 1, K % 64 == 0, N % 64 == 0.
struct GemmBf16ProArgs {
    const void* A; int lda; int a_f32;  // a_f32 = 1: fp32 rows, staged as RNE_bf16((x - mean) rstd) with mom; 0: bf16 rows, staged as they are
    const float* mom;                   // a_f32: [M] (mean, rstd) pairs (launch_row_moments)
    const bf16* W;                      // [N, K] row-major (the kernel's packed order)
    const float* bias;                  // [N]
    const float* R;                     // fp32 residual [M, N] or null; may be Cf
    float* Cf; bf16* Cb;                // exactly one: fp32 or RNE bf16 store, [M, N]
    int M, N, K, act;                   // act: ACT_NONE or ACT_GELU (erf), on acc + bias
    int tile;                           // 0: the launcher picks; 1 / 2: 64 x 64 / 128 x 128 tiles (the bits do not depend on it)
    int nt_n;                           // (launcher)
};
int launch_gemm_bf16_pro(const GemmBf16ProArgs& a, hipStream_t s);
// mom[row] = (mean, 1 / sqrt(var + eps)) of fp32 rows of C <= 1024 channels, two-pass
int launch_row_moments(const float* x, int rows, int C, float eps, float* mom, hipStream_t s);

template <typename T>
int launch_ln_rows(float* h, int ldh, int M, int D, const float* pre_add, int n_pre_rows, const float* gamma,
                   const float* beta, T* out, int ldo, hipStream_t s);
template <typename TI, typename T>
int launch_ln_film_silu_rows(const TI* y, int ldy, int M, int D, const float* gamma, const float* beta,
                             const float* film, int film_ld, int film_off, int frames, int bmod, T* out, int ldo,
                             hipStream_t s);
template <typename T>
int launch_concat_ln_rows(const ConcatSegs& sg, int M, const float* gamma, const float* beta, T* out, int ldo, int Ppad,
                          hipStream_t s);
template <typename TI, typename T>
int launch_im2col3_rows(const TI* x, int ldx, int B, int frames, int Cin, T* out, int ldo, hipStream_t s, const int* lens = nullptr);
template <typename T>
int launch_temb_rows(const int64_t* t, int B, int dim, T* out, int ldo, hipStream_t s);
template <typename T>
int launch_pack_cols(const float* x, int ldx, int M, int c0, int w, int wpad, float scale, T* out, int ldo, float* outf,
                     int ldof, hipStream_t s);
// (guidance scale of clip b: scale[b * scale_row], device fp32; scale_row 0 = one value for the batch, 1 = one per clip)
int launch_cfg_mix(const float* o, int ldo, int Mc, int cond_row0, int frames, int w, int has_null, const float* scale, int scale_row,
                   float* eps, int lde, int c0, const float* x, int ldx, const float* c1, const float* c2, float* x0,
                   int ldx0, hipStream_t s);
// The mix of a doubled batch under a guidance schedule (rowops.hip): sched = [gain row 0 [n_steps] | gain row 1 [n_steps] | phi 0, phi 1]
// (device fp32), m = the row this encoder reads, t[b * t_row] the clip's model timestep (clamped into the table).  rescale = false: one
// launch, which also writes x0.  rescale = true (the host's phi_m > 0): a second launch scales eps by the clip's std ratio over its
// lens[b] (null: frames) valid rows and writes x0; part = 4 fp64 per token row of scratch.
int launch_cfg_mix_sched(const float* o, int ldo, int Mc, int cond_row0, int frames, int w, const float* scale, int scale_row,
                         const int64_t* t, int t_row, const float* sched, int n_steps, int m, bool rescale, const int* lens, double* part,
                         float* eps, int lde, int c0, const float* x, int ldx, const float* c1, const float* c2, float* x0, int ldx0,
                         hipStream_t s);

// ---- token-per-lane fused Linear, K = 512, bf16 (tl_linear.hip) ------------------------------
// Row-indexed tensors are TILED (layouts at the top of tl_linear.hip; helpers below) and padded to 128-row blocks.
struct TlArgs {
    const void* X; int ldx;        // bf16 tiled [M, K] input (ldx = its width in features)
    const void* W;                 // bf16 [N, K], rows pi-permuted inside every 32-row tile (tl_weight_src_row)
    const float* bias;             // [N] or null
    const float* R; int ldr;       // fp32 tiled residual [M, N] or null (ldr unused)
    float* Cf; int ldcf;           // fp32 out or null: tiled [M, N], or row-major with ldcf when cf_rowmajor
    int cf_rowmajor;
    void* Ct; int ldct;            // bf16 tiled out [M, N] or null (ldct unused)
    int half_row0;                 // FiLM prologue: rows >= half_row0 index the batch as (row - half_row0) / frames
    int M, N, K, act;              // K = 512 or 1024
    const float* gamma; const float* beta;                          // prologue LayerNorm affine [K] (pro 1 / 3)
    const float* film; int film_ld, film_off, frames, bmod;         // pro 2: FOLDED FiLM table rows [A | B] (launch_film_fold)
    const float* row_const; int n_const_rows;                       // epilogue: + row_const[n] for rows < n_const_rows
    // prologue 3 (K = 1024 only): the row is the virtual concat [X(512) | X1(256) | X2(128) | X3(128, may be null)]
    // of four tiled tensors (transformer.py:304-312), LayerNorm over the first kreal columns; gamma/beta zero-padded
    const void* X1; int ld1; const void* X2; int ld2; const void* X3; int ld3; int kreal;
    int tiles_per_block;                                            // 32-feature tiles per blockIdx.y (set by the launcher)
    int stag_groups, stag_sleep;                                    // first-round start stagger (set by the launcher), as Tl2FfnArgs
    int rev;                                                        // 1: token blocks in descending order (tl_block_index, tl_common.h)
    int rot;                                                        // tl2 rolling loop: block b starts its weight stream at tile (b / 8) % tiles (set by the launcher)
    // residual stream as two bf16 planes (tl_common.h): Rlo != null -> the residual is (R reinterpreted as the bf16 hi plane) + Rlo;
    // Clo != null -> the result leaves as Ct (hi plane) + Clo (lo plane) and Cf is not written.  Planes are tiled bf16 [M, N].
    const void* Rlo; void* Clo;
    int tls_nb0, tls_tb1;                                           // window-chain kernels (tl_small.hip): 32-token blocks of the first row
                                                                    // range / first block of the second one (set by the launcher)
    int dbg;                                                        // ablation bits (bench only)
    unsigned long long* clk;                                        // clock probe output {shader cycles, 100 MHz ticks} or null
    unsigned long long* trace;                                      // block timeline (bench only): 4 words per block, or null
};
// pro: 0 = plain rows, 1 = LayerNorm, 2 = LayerNorm -> FiLM -> SiLU (StylizationBlock), 3 = concat + LayerNorm (feat_proj.0)
int launch_tl_linear(const TlArgs& a, int pro, hipStream_t s);
// the FiLM prologue (pro 2) of launch_tl_linear stages the folded rows of at most TL_MAXCLIP = 6 clips per 128-token block: true when a
// launch over `bmod` clips of `frames` frames stays within that (clips of 26 frames and more at any batch, shorter ones up to 6 clips)
bool tl_linear_film_clips_ok(int frames, int bmod);
// window-chain batches (tl_small.hip): 32 tokens per block, one tile per wave, weights straight from the fragment-ordered copy
// (a.W as for launch_tl2_linear; pro 1 / 3: a.bias = d, a.row_const = c of the folded LayerNorm).  Rows = frames * bmod, or two
// CFG halves of that many rows with the second one starting at row M - frames * bmod.
bool tls_linear_supported(const TlArgs& a, int pro);
// their FiLM prologue (pro 2) stages at most TLS_MAXCLIP = 4 clips per 32-token block: clips of 11 frames and more at any batch, shorter ones up to 4 clips
bool tls_film_clips_ok(int frames, int bmod);
int launch_tls_linear(const TlArgs& a, int pro, hipStream_t s);
int tl_weight_src_row(int r);

// ---- second generation (tl2.hip): LDS-DMA weight stream from FRAGMENT-ORDERED weights -------------------------------
// same arguments as launch_tl_linear, except that a.W is the fragment-ordered copy of the weight (tl2_frag_index)
int launch_tl2_linear(const TlArgs& a, int pro, hipStream_t s);
extern int g_tl_last_variant;          // test helper (dsh_debug_last_tl_variant): family the last token-per-lane Linear launch selected
// element index of stored row n (inside 32-row tile nt; rows pi-permuted as for tl_linear) / column k of a [N, K] weight
size_t tl2_frag_index(int K, int nt, int n, int k);
// FFN branch of a decoder layer in one launch: h <- h + Sty(GELU(h16 W1^T + b1) W2^T + b2)   (transformer.py:169-181)
struct Tl2FfnArgs {
    const void* X;                       // bf16 tiled [M, 512]: the layer's residual stream (bf16 shadow)
    const void* Wffn;                    // weight stream: 80 chunks of 32 KB in phase order (W1 tiles / W2 K chunks interleaved, W3 tiles; tl2.hip)
    const float* b1; const float* b2; const float* b3;
    const float* film; int film_ld, film_off, frames, bmod, half_row0;   // folded FiLM rows [A | B] of ffn.proj_out
    const float* R; float* Cf; void* Ct; // h in (fp32 tiled), h out, bf16 shadow out
    const float* row_const; int n_const_rows;
    int M;
    unsigned long long* trace;           // block timeline (bench only) or null
    unsigned long long* clk;             // phase probe (bench only): 8 words per block, or null
    int stag_groups, stag_sleep;         // first-round start stagger (set by the launcher): block b < 256 sleeps (b % groups) * sleep * 8 k cycles
    int rev;                             // 1: token blocks in descending order (tl_block_index, tl_common.h)
    const void* Rhi; const void* Rlo; void* Clo;   // hi / lo planes of the residual stream (tl3_ffn_kernel only): Rhi != null replaces R / Cf
};
void tl_stagger_config(int which, int* groups, int* sleep);   // DSH_STAGGER (tl2.hip)
bool tl2_ffn_supported(int M, int frames, int bmod);
int launch_tl2_ffn(const Tl2FfnArgs& a, hipStream_t s);
// third generation (tl3_ffn.hip): same arguments, Wffn in the version-3 stream order (K-outer Linear3 in two passes)
int launch_tl3_ffn(const Tl2FfnArgs& a, hipStream_t s);
bool tl3_ffn_supported(int M, int frames, int bmod, bool planes);   // the gate Denoiser::run_encoder uses for generation 3
// the 80-chunk weight stream of the fused FFN kernels from pi-permuted row-major bf16 weights ([1024,512], [512,1024], [512,512]);
// version 2: tl2_ffn_kernel, 3: tl3_ffn_kernel; `st` receives 80 * 16384 elements
void tl_pack_ffn_stream(int version, const uint16_t* w1p, const uint16_t* w2p, const uint16_t* w3p, uint16_t* st);
// the operands of one token-per-lane Linear from its fp32 weight W [N, K] (bias [N], gamma / beta [K]: null = none), K zero padded to Kp
// and N to Np = round_up(N, 32); the one packer of finalize() and of the op-level entries (tl2.hip).  perm / frag [Np, Kp] bf16: the
// pi-permuted rows (never folded: operand of launch_tl_linear and of tl_pack_ffn_stream) and the fragment-ordered copy (launch_tl2_linear,
// launch_tls_linear), folded with the LayerNorm when gamma is given; fc / fd [Np] then receive its c and d vectors (else they may be null)
void tl_pack_linear(const float* W, const float* bias, int N, int K, int Kp, const float* gamma, const float* beta, uint16_t* perm, uint16_t* frag,
                    float* fc, float* fd);

// ---- tiled-layout helpers (rowops.hip).  bf16 tiles: 32 tokens x 16 features; fp32: lane-native 32 x 32 blocks ----
// row-major [M, w] (ld, element type TS = float or bf16) -> bf16 tiled [Mpad, Wd]; columns >= w are zero filled
template <typename TS>
int launch_tile_rows_bf16(const TS* src, int ld, int M, int w, void* dst, int Wd, hipStream_t s);
int launch_untile_rows_bf16(const void* src, int Wd, int M, int w, void* dst_bf16, int ld, hipStream_t s);
// the given expression track of a gesture-only condition [B frames, E] fp32 -> fp32 rows x0 [.., ld] (pad columns zero) and, x16 != null, the
// tiled bf16 operand [.., 128] exactly as launch_tile_rows_bf16 rounds it; lens != null: frames beyond a clip's length are written as zero
int launch_pack_expr_track(const float* src, int E, int B, int frames, const int* lens, float* x0, int ld, void* x16, hipStream_t s);
// columns [c_lo, c_hi) of dst [M, C] <- src [M, src_ld] (its first c_hi - c_lo columns), or 0 when src is null
int launch_fill_cols(float* dst, int C, size_t M, int c_lo, int c_hi, const float* src, int src_ld, hipStream_t s);
int launch_tile_rows_f32(const float* src, int ld, int M, float* dst, int Wd, hipStream_t s);
int launch_untile_rows_f32(const float* src, int Wd, int M, float* dst, int ld, hipStream_t s);
// FiLM table rows [scale | shift] -> folded [A | B] coefficients of the token-per-lane StylizationBlock prologue (in place)
int launch_film_fold(float* tab, int ld, int B, int nblk, int D, const float* gamma, const float* beta, hipStream_t s);
// round 6: the same from the DISTINCT embedding rows: dst[b] = fold(src[idx[b]]) for b < B (idx == null: identity; fold == 0: plain copy)
int launch_film_expand(const float* src, int ld, const int* idx, float* dst, int B, int nblk, int D, const float* gamma, const float* beta,
                       int fold, hipStream_t s);
int launch_gather_rows_f32(const float* src, int ld, const int* idx, float* dst, int ldd, int B, int w, hipStream_t s);
// layer-0 seed of the tiled residual stream from the row-major joint_embed output h0 [Mc, 512]:
// rows [0, Mc) (CFG-null half) = h0 + c, rows [row1, row1 + Mc) (conditional half) = h0; fp32 tiled + bf16 tiled shadow.
// has_null == 0: only rows [0, Mc) = h0.
int launch_seed_stream(const float* h0, int Mc, int D, const float* c, int has_null, int row1, float* h, void* h16, hipStream_t s,
                       void* hlo = nullptr);      // hlo != null: the stream is seeded as (h16 = hi, hlo = lo) planes and h is not written
// round 6 (tl_embed.hip): the same seed straight from the tiled bf16 channels of x — joint_embed + bias + PE + null constant + plane split
// in one launch; x_tiled [Mc, 16 nf] (nf = 7 or 9), wfrag = fragment-ordered [512, 16 nf] weight
void tl_joint_pack_weight(const float* w, int cin, int nf, uint16_t* fr);     // joint_embed [512, cin] fp32 -> wfrag (512 * 16 nf bf16)
int launch_tl_joint(const void* x_tiled, int nf, const void* wfrag, const float* bias, const float* pe, int frames, const float* cnull,
                    int Mc, int row1, void* hi, void* lo, hipStream_t s);
// round 6 (tl_aud.hip): encoder_aud behind its attention (two StylizationBlocks + FFN at D = 128) in one launch; Y bf16 [Mc,128] and X2 fp32
// [Mc,128] row-major, Wst = tl_aud_pack_stream, bias = [proj_out(sa) 128 | linear1 1024 | linear2 128 | proj_out(ffn) 128], film = FOLDED rows
// [A1 | B1 | A2 | B2] (128 each) of embedding row (token / frames) % bmod
void tl_aud_pack_stream(const float* ws1, const float* w1, const float* w2, const float* ws2, uint16_t* st);
void tl_aud_pack_audio_proj(const float* w, uint16_t* st);     // audio_proj [256,256] -> 4 chunks per motion encoder behind the 18 (read by launch_tl_aproj)
int launch_tl_aud_tail(const void* Y, const float* X2, const void* Wst, const float* bias, const float* film, int film_ld, int bmod, int frames,
                       int Mc, float* out_f, void* out_b, int ld_b, hipStream_t s);
// audio_proj of up to two motion encoders from the row-major bf16 [Mc, 256] operand straight into their tiled [Mc, 256] concat operands
// (tl_embed.hip); wfrag = tl_aud_pack_audio_proj per encoder (128 KB apart), bias [n_enc][256]
int launch_tl_aproj(const void* x256, const void* wfrag, const float* bias, int n_enc, void* out0, void* out1, int Mc, hipStream_t s);
// row-major fp32 [M, w] <-> hi / lo bf16 planes in the tiled layout (test helpers of capi.hip)
int launch_tile_rows_hilo(const float* src, int ld, int M, int w, void* hi, void* lo, int Wd, hipStream_t s);
int launch_untile_rows_hilo(const void* hi, const void* lo, int Wd, int M, int w, float* dst, int ld, hipStream_t s);

int launch_interp_time(const float* x, int B, int Tin, int C, float* y, int Tout, hipStream_t s);
// per-row frame counts on both sides (DEVICE int32 [B]): row b = the dense call on (lens_in[b], lens_out[b]), 0 behind lens_out[b]
int launch_interp_time_ragged(const float* x, int B, int Tin, int C, float* y, int Tout, const int* lens_in, const int* lens_out, hipStream_t s);
int launch_affine_cols(const float* x, size_t n, int C, const float* mean, const float* stdv, float* y, hipStream_t s);
// BEAT results tail (rotation.hip): standardised axis-angle <-> standardised Euler 'XYZ' degrees per joint triple, rows addressed by a stride
// (elements), optional per-clip lengths (device int32, `frames` rows per clip: rows behind a clip's length are written as zeros)
int launch_axis_angle_to_euler(const float* x, long long ldx, long long rows, int joints, const float* mean_aa, const float* std_aa,
                               const float* mean_e, const float* std_e, float* y_std, long long ld_std, float* y_deg, long long ld_deg,
                               const int* lengths, int frames, hipStream_t s);
int launch_euler_to_axis_angle(const float* x, long long ldx, long long rows, int joints, const float* mean_e, const float* std_e,
                               const float* mean_aa, const float* std_aa, float* y, long long ldy, const int* lengths, int frames,
                               hipStream_t s);
// Forward kinematics (kinematics.hip): world positions [rows, 3 J] (and world rotations [rows, 9 J], nullable) of a rotation-only skeleton
// from the standardised channel triples, and the vector-Jacobian product of the positions (axis-angle input).  All skeleton arrays are
// device buffers; strides in elements; lengths / frames as above.  kind 0: axis-angle, 1: Euler 'XYZ' degrees.
struct FkSkeleton {
    int J, Jc;                     // joints, driven joints (channel triples)
    const int* parents;            // [J], parents[0] = -1, parents[j] < j
    const float* offsets;          // [J, 3]
    const int* channel_joint;      // [Jc]: the joint channel triple i drives
    const float* rest_rot;         // [J, 3, 3]: the rotation of a joint no channel drives
    const int* joint_channel;      // [J]: the inverse map, -1 where undriven
};
int launch_fk_positions(const float* x, long long ldx, long long rows, int kind, const float* mean, const float* stdv, const FkSkeleton& sk,
                        float* pos, long long ld_pos, float* wrot, long long ld_wrot, const int* lengths, int frames, hipStream_t s);
int launch_fk_positions_vjp(const float* x, long long ldx, long long rows, const float* mean, const float* stdv, const FkSkeleton& sk,
                            const float* g, long long ldg, float* dx, long long lddx, const int* lengths, int frames, hipStream_t s);

// linear ("efficient") self-attention core: y = softmax_ch(Q) (softmax_time(K)^T V)   (transformer.py:122-128)
// lens (device int32, nullable): ragged batch — clip b has lens[b % lmod] valid frames out of `frames` (the padded stride); frames beyond
// them enter neither the K softmax nor k^T v.  Null: every frame is valid, the launch is the one it always was.
template <typename T>
int launch_linear_attention(const T* qkv, int ldq, int nbatch, int frames, int D, int head_dim, T* y, int ldy,
                            hipStream_t s, const int* lens = nullptr, int lmod = 0);
// cross-attention core (LinearTemporalCrossAttention, transformer.py:146-166): q [B,T,D] (ldq), kv [B,N,2D] = (k | v) (ldkv), fp32
int launch_linear_cross_attention(const float* q, int ldq, int nbatch, int frames, const float* kv, int ldkv, int frames_kv, int D,
                                  int head_dim, float* y, int ldy, hipStream_t s);
int launch_silu_f32(const float* x, float* y, size_t n, hipStream_t s);
// bf16 tiled qkv [M, 3D] -> bf16 tiled y [M, D]; batch b starts at row b * frames (b < half_batches) or
// half_row0 + (b - half_batches) * frames
bool linear_attention_sty_f32_supported(int frames, int D, int head_dim, int ldq, int ldy);
int launch_linear_attention_sty_f32(const float* qkv, int ldq, int nbatch, int frames, int D, float* s_out, int ldy, const float* film, int film_ld, int film_off,
                                    int bmod, hipStream_t s, const int* lens = nullptr, int lmod = 0);
// (lens: one entry per clip of a CFG half, [half_batches])
int launch_linear_attention_tiled(const void* qkv, int nbatch, int half_batches, int half_row0, int frames, int D, void* y,
                                  hipStream_t s, int rev = 0, const int* lens = nullptr);

// ---- sampler element-wise kernels (sampler_kernels.hip) ------------------------------------
struct DdimStepArgs {
    float* x;              // [n] in/out sample
    const float* eps;      // [n] model output
    float* x0_out;         // [n] pred_xstart or null
    float c1, c2;          // sqrt(1/abar), sqrt(1/abar - 1)          (fp64 table -> fp32)
    float sqrt_ab_prev;    // sqrt_f32(f32(abar_prev))
    float sqrt_1m_ab_prev; // sqrt_f32(1 - f32(abar_prev))
    // eta != 0 (gaussian_diffusion.py:1011-1032): coef_eps = sqrt(1 - abar_prev - sigma^2) multiplies the re-derived eps (eta = 0:
    // = sqrt_1m_ab_prev), and sigma * noise1 is added (sigma already carries the t != 0 mask); noise1 == null: no such term
    float coef_eps, sigma;
    const float* noise1;   // [n] N(0,1): the randn_like of the step
    // RePaint blend (gaussian_diffusion.py:1034-1056); mask == null disables it
    const uint8_t* mask;   // [n] bool
    const float* gt;       // [n]
    const float* noise2;   // [n] N(0,1) for the gt branch
    int blend;             // 1: linear cross-fade on the first overlap_len frames
    int tail_blend = 0;    // 1 (with blend): the mirrored cross-fade on the last overlap_len frames (windows pinned at both ends; 2 overlap_len <= frames)
    int clip;              // clamp x0 to [-1,1] before re-deriving eps (clip_denoised)
    int overlap_len, frames, channels;
    size_t n;
    // --same_overlap_noisy: tail_in [B, overlap_len, C] replaces the noised gt on the out-painted frames (null: off / first
    // window); tail_out [B, overlap_len, C] receives the last overlap_len frames of the updated sample (null: off)
    const float* tail_in; float* tail_out;
    // channel range [c_lo, c_hi) of the update (0 / 0 = all): the expression and the gesture channels of a sample never interact in the sampler's
    // element-wise updates, so the two encoders' chains may advance on their own streams (sampler.hip, pipelined small-batch loop)
    int c_lo = 0, c_hi = 0;
    // second != 0: the step is one second-order DPM-Solver++(2M) update in the data-prediction form, eta = 0: x0 as above (clamped when
    // clip is on), D = x0 + G (x0 - x0_prev), x <- A x + Bc D, then the RePaint branch unchanged.  x0_out (required) holds x0_prev on entry
    // and x0 on return, in the columns [c_lo, c_hi).  A, Bc, G: solver_coeffs() of sampler.h (fp64 -> fp32).  coef_eps and sigma are not read;
    // noise1, tail_in and tail_out must be null.
    int second = 0;
    float A = 0.f, Bc = 0.f, G = 0.f;
};
int launch_ddim_step(const DdimStepArgs& a, hipStream_t s);
int launch_undo_step(float* x, const float* noise, float sqrt_1m_beta, float sqrt_beta, size_t n, hipStream_t s, int channels = 0, int c_lo = 0, int c_hi = 0);
struct DdpmStepArgs {
    float* x; const float* eps; const float* noise; float* x0_out;
    float c1, c2, coef1, coef2, sigma;   // sigma = exp(0.5*logvar) or 0 at t == 0
    int clip;
    size_t n;
    int channels = 0, c_lo = 0, c_hi = 0;   // channel range of the update (c_hi <= c_lo: all), as DdimStepArgs
};
int launch_ddpm_step(const DdpmStepArgs& a, hipStream_t s);
// ---- soft constraints while sampling: per column c of clip b with L = lens[b] frames (frames if null), on the signal z,
//   log p = -1/2 sum_t W (z[t] - Y)^2  - 1/2 vel[c] sum_{t=0..L-2} (z[t+1] - z[t])^2  - 1/2 acc[c] sum_{t=1..L-2} (z[t+1] - 2 z[t] + z[t-1])^2
//   g[t]  = scale * d log p / d z[t]      (a five-point stencil; 0 at frames >= L)
// Every term is local to its column: the column ranges of the step launches and the two encoders' chains keep working.
struct GuideArgs {
    const float* target = nullptr;   // Y [n], addressed like x; null: 0
    const float* weight = nullptr;   // W [n] >= 0, addressed like x; null: no attraction term
    const float* vel = nullptr;      // [channels] or null
    const float* acc = nullptr;      // [channels] or null
    const int* lens = nullptr;       // [B] per-clip frame counts (ragged batch) or null; the guided launches leave frames >= lens[b] unwritten
    float scale = 1.f;               // s_k of the step's spaced level
    int space = 0;                   // GUIDE_XT: z = the noisy sample (the reference's cond_fn(x, t)); GUIDE_X0: z = the step's pred_xstart
    float sqrt_1m_ab = 0.f;          // DDIM (condition_score, gaussian_diffusion.py:670-673): sqrt_f32(1 - f32(abar))
    float post_var = 0.f;            // DDPM (condition_mean, :654-657): f32(posterior_variance)
};
enum GuideSpace { GUIDE_XT = 0, GUIDE_X0 = 1 };
// g[b, t, c] for the columns [c_lo, c_hi) (0 / 0: all) of z [B, frames, channels]; other columns of g are not written
int launch_guidance_grad(const float* z, float* g, int B, int frames, int channels, int c_lo, int c_hi, const GuideArgs& ga, hipStream_t s);
// The guided forms of the two steps, each one pass.  DDIM (also a.second): x0 as in launch_ddim_step (clipped when a.clip), e = (c1 x - x0) / c2,
// e' = e - sqrt_1m_ab g, x0' = c1 x - c2 e', then the parent's update from x0' (eta term, x0_out / history, RePaint select, saved tails).
// DDPM: mean' = mean + post_var g.  a.n must be B * frames * channels (whole clips: the stencil walks a clip's frames).
int launch_guided_ddim_step(const DdimStepArgs& a, const GuideArgs& ga, hipStream_t s);
int launch_guided_ddpm_step(const DdpmStepArgs& a, int frames, const GuideArgs& ga, hipStream_t s);
int launch_fill_i64(int64_t* p, int64_t v, size_t n, hipStream_t s);
// p[0, n) = host[0, n) in stream order (values passed as launch arguments: the host array may be reused at once, no sync)
int launch_store_values_f32(float* p, const float* host, int n, hipStream_t s);
int launch_fill_f32(float* p, float v, size_t n, hipStream_t s);
int launch_fill_step(int64_t* t, float* c1, float* c2, int64_t* level, int64_t tv, float c1v, float c2v, int64_t lv, int n, hipStream_t s);
struct LevelCopyArgs {
    char* work[4]; size_t bytes[4]; size_t off[4]; int nseg;
    char* slots; size_t stride; const int64_t* level; int restore;
};
int launch_level_copy(const LevelCopyArgs& a, hipStream_t s);
// Philox4x32-10 + Box-Muller standard normals; element i uses counter (offset + i/4)
int launch_philox_randn(float* out, size_t n, uint64_t seed, uint64_t offset, hipStream_t s);
// per-row streams: row b of `rows` x n_row values uses key `seed`, counter = (in-row quad index, row_keys[b]) (device array)
// row_lens (device, nullable): ragged rows — row b advances by row_lens[b] * channels / 4 counters per draw instead of `offset`
int launch_zero_padded_frames(float* x, const int* lens, int B, int frames, int channels, hipStream_t s);
int launch_philox_randn_rows(float* out, int rows, size_t n_row, uint64_t seed, uint64_t offset, const uint64_t* row_keys,
                             hipStream_t s, const int* row_lens = nullptr, uint64_t draw = 0, int channels = 0,
                             const uint64_t* row_seeds = nullptr);      // (device, nullable: row b's Philox key in place of `seed`)
// q_sample (sampler_kernels.hip): out = a[b] x0 + s[b] n per element of row b; n = noise, or (noise null) the Philox draw the fields below
// address exactly as launch_philox_randn (row_keys null: offset + global quad) / launch_philox_randn_rows do.  All pointers device.
struct QSampleArgs {
    float* out; const float* x0; const float* noise;
    const float *a, *s;                    // [B] coefficient pairs
    size_t n; int frames, channels;
    int c_lo, c_hi, fixed_from;            // columns written (c_hi <= c_lo: all); columns >= fixed_from copy x0 (-1: none)
    uint64_t seed, offset; const uint64_t* row_keys; size_t row_quads; const int* row_lens; uint64_t draw; const uint64_t* row_seeds;
    int vec;                               // set by launch_q_sample: whole quads as float4 (no window, no fixed columns, no lengths, aligned)
};
int launch_q_sample(const QSampleArgs& a, hipStream_t s);
// keep mask of an edit [B, T, C]: 0 inside any of row b's frame ranges frames[b, nf, 2] or any column range cols[nc, 2] (device), 1 elsewhere
int launch_region_mask(const int* frames, int nf, const int* cols, int nc, int B, int T, int C, uint8_t* keep, hipStream_t s);
// window hand-off of live chains on a slot table tails [S, L, C]: gt [R, T, C] <- (tails[slot_idx[r]] | 0), mask [R, T, C] <- (1 | 0) ...
int launch_chain_handoff(const float* tails, int S, const int* slot_idx, int R, int T, int L, int C, float* gt, uint8_t* mask, hipStream_t s);
// ... and tails[slot_idx[r]] <- the last L valid frames of x [R, T, C] (lens nullable: every row has T).  slot_idx / lens: device arrays.
int launch_chain_save_tail(const float* x, const int* lens, const int* slot_idx, int S, int R, int T, int L, int C, float* tails, hipStream_t s);
// Synchronised window batches: row b of x [B, frames, channels] shares its first L frames with the last L valid frames of row left[b]
// (-1: no left neighbour); both copies become a (1 - w) + r w, w = linspace(0, 1, L)[j], in place, on columns [c_lo, c_hi) ((0, 0): all).
// left_dev / lens_dev (nullable: every row has `frames`): device arrays.  check_window_sync() is the host-side condition of the in-place
// update (0, or -1 with the reason in err): indices in range and injective, left[b] != b, every used row holds L frames inside its length,
// a row used at both ends 2 L.
int check_window_sync(const int32_t* left, const int32_t* lens, int B, int T, int L, std::string& err);
int launch_window_sync(float* x, int B, int frames, int channels, const int* left_dev, const int* lens_dev, int L, int c_lo, int c_hi,
                       hipStream_t s);

}  // namespace dsh
