// The DSH_* runtime switches: ONE table of every environment variable the library reads, the typed accessors every reader goes
// through, and the derivations that more than one reader shares.  This is the only file under csrc/ that reads the environment.
// INTEGRATION.md section 4b lists the same entries for users; dsh_switch_count / _info / _read (switches.hip) expose them to tests.
//
// WHEN a switch is read:
//   PROCESS  latched by the first read in the process (the accessor caches it, per switch): flipping it later changes nothing, so
//            an A/B over it needs a fresh process per arm
//   CONTEXT  read when a denoiser context is constructed (dsh_create): a new context sees a new value
//   CALL     read on every call / launch / evaluation that uses it: one environment lookup per read, nothing cached
// A few switches have a second reader with another moment; the entry's text says so and that reader uses the *_now / latch it names.
//
// CLASS: PRODUCT a deployment knob; AB_EXACT an A/B whose arms give bit-identical results; AB_ROUNDOFF an A/B whose arms differ by
// floating-point round-off (another kernel family or summation order); BENCH a measurement hook, results may be garbage.
//
// Parsing, the same for every integer switch: the value is what atoi gives (strtol, base 10), so an empty or non-numeric value is 0 —
// a default-on switch is therefore OFF when it is set to the empty string — and an unset switch takes the default of its entry.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

namespace dsh {

enum SwitchKind : int { SWK_INT = 0, SWK_FLAG = 1, SWK_STR = 2 };          // integer / present-or-absent / string
enum SwitchWhen : int { SWW_PROCESS = 0, SWW_CONTEXT = 1, SWW_CALL = 2 };
enum SwitchClass : int { SWC_PRODUCT = 0, SWC_AB_EXACT = 1, SWC_AB_ROUNDOFF = 2, SWC_BENCH = 3 };

//   id, variable, kind, default, when, class, meaning
#define DSH_SWITCH_TABLE(X)                                                                                                                      \
    X(DUAL, "DSH_DUAL", INT, "3", CONTEXT, PRODUCT, "most sub-batch streams of a large batch: 0 one stream, 1 two, n at most n (1 .. 8); results identical") \
    X(DUAL_LAG, "DSH_DUAL_LAG", INT, "3", CONTEXT, PRODUCT, "stream i + 1 starts this many token-per-lane launches behind stream i; the sampler reads it again per loop (CALL)") \
    X(DUAL_ROWS, "DSH_DUAL_ROWS", INT, "21500 (fp32: 2900)", CONTEXT, PRODUCT, "token rows per sub-batch stream; overrides only when positive") \
    X(DUAL_MIN_ROWS, "DSH_DUAL_MIN_ROWS", INT, "12288 (fp32: 4096)", CONTEXT, PRODUCT, "smallest batch (token rows) split over sub-batch streams; overrides only when positive") \
    X(PIPE, "DSH_PIPE", INT, "1", CALL, AB_EXACT, "sampling loops: the two encoders on two streams, the gesture encoder one step behind; 0 in sequence") \
    X(PIPE_ROWS, "DSH_PIPE_ROWS", INT, "64499", PROCESS, PRODUCT, "token rows below which a loop runs ONE batch with two encoder streams; latched in the sampler, read afresh (CONTEXT) by the sub-batch splitter") \
    X(NO_GRAPH, "DSH_NO_GRAPH", FLAG, "unset", CALL, PRODUCT, "present (any value, 0 included): small-batch evaluations are not replayed from a hipGraph") \
    X(GRAPH_ROWS, "DSH_GRAPH_ROWS", INT, "4096", PROCESS, PRODUCT, "token rows up to which a sampling loop replays its evaluations from a hipGraph") \
    X(LEVEL_CACHE, "DSH_LEVEL_CACHE", INT, "1", CALL, AB_EXACT, "x-independent part of an evaluation once per timestep level; 0 on every step") \
    X(LEVEL_PREFETCH, "DSH_LEVEL_PREFETCH", INT, "1", CALL, AB_EXACT, "that part ahead of the loop on a side stream; 0 inline at a level's first use") \
    X(TL2, "DSH_TL2", INT, "1", CONTEXT, AB_ROUNDOFF, "token-per-lane Linears: 0 first generation, 1 LDS-DMA kernels, 2 LDS-DMA everywhere (fp32 residual); dsh_op_tl_linear reads it per CALL") \
    X(TL2_ROLL, "DSH_TL2_ROLL", INT, "1", CALL, AB_EXACT, "rolling main loop of q|k|v / feat_proj.1 / ffn.linear2; 0 the round-2 loop") \
    X(TL2_ROT, "DSH_TL2_ROT", INT, "0", CALL, AB_EXACT, "rolling launches walk the weight tiles in a per-block rotated order (measured neutral)") \
    X(TL2_KSKIP, "DSH_TL2_KSKIP", INT, "1", CALL, AB_EXACT, "feat_proj.1 skips the trailing all-zero fragments of the concat row; 0 multiplies all 64") \
    X(TL2_HL, "DSH_TL2_HL", INT, "1", CONTEXT, AB_EXACT, "LDS-DMA kernels for the two residual-carrying Linears on hi / lo planes; 0 first generation") \
    X(FFN_FUSE, "DSH_FFN_FUSE", INT, "1", CONTEXT, AB_ROUNDOFF, "FFN branch as one fused launch; 0 three launches") \
    X(FFN_V, "DSH_FFN_V", INT, "3", CONTEXT, AB_ROUNDOFF, "fused FFN kernel generation: only 2 selects tl2_ffn_kernel, anything else tl3_ffn_kernel; dsh_op_tl2_ffn and the profiler's class text read it per CALL") \
    X(FFN_PC, "DSH_FFN_PC", INT, "1", CALL, AB_EXACT, "fused FFN phase C: 0 the round-4 loop, 1 pipelined across the phase boundary, 2 also pass-B epilogues early (clamped to 0 .. 2)") \
    X(FFN_PB, "DSH_FFN_PB", INT, "1", CALL, AB_EXACT, "fused FFN last stage (& 3): bit 0 hi plane kept in registers, bit 1 pass-B residual requested early; the denoiser's profiler byte count latches it") \
    X(FFN_X_IS_HI, "DSH_FFN_X_IS_HI", INT, "0", CALL, BENCH, "dsh_op_tl2_ffn on hi / lo planes: the input IS the hi plane of the residual, as in the denoiser's layers") \
    X(FFN_REPEAT, "DSH_FFN_REPEAT", INT, "0", CALL, BENCH, "dsh_op_tl2_ffn launches its kernel this many extra times (results unchanged)") \
    X(HILO, "DSH_HILO", INT, "1 (op entries: 0)", CONTEXT, AB_ROUNDOFF, "bf16 residual stream as hi + lo planes; 0 fp32 + bf16 shadow.  The op entries read it per CALL and take unset as OFF (hilo_denoiser / hilo_op below)") \
    X(TLS, "DSH_TLS", INT, "1", CONTEXT, AB_EXACT, "window-chain batches on the 32-token-block kernels of tl_small.hip; 0 off") \
    X(TLS_ROWS, "DSH_TLS_ROWS", INT, "per instantiation", CONTEXT, AB_EXACT, "token rows per launch up to which those kernels are used; overrides only when positive") \
    X(REV, "DSH_REV", INT, "1", CONTEXT, AB_EXACT, "alternate the row order of consecutive large token-per-lane launches; 0 off") \
    X(STAGGER, "DSH_STAGGER", STR, "unset", PROCESS, AB_EXACT, "\"groups,sleep[,mask]\" (%d,%d,%d): staggered first-round block start; mask bit 0 fused FFN, 1 q|k|v, 2 the other Linears") \
    X(SPLIT_AT, "DSH_SPLIT_AT", STR, "unset", PROCESS, BENCH, "\"c1,c2,...\": explicit sub-batch boundaries (clip indices); the list is latched, the once-only warning looks at its presence per CONTEXT") \
    X(DBG_SKIP, "DSH_DBG_SKIP", INT, "0", CONTEXT, BENCH, "mask of launches of a layer that are not issued (results are garbage; warns once)") \
    X(EMB_DEDUP, "DSH_EMB_DEDUP", INT, "1", CALL, AB_ROUNDOFF, "embedding Linears on the distinct (timestep, speaker) rows; 0 every clip's row (bit-identical up to 16 rows)") \
    X(JOINT_FUSE, "DSH_JOINT_FUSE", INT, "1", CALL, AB_EXACT, "layer-0 seed as one token-per-lane launch; 0 pack_cols + GEMM + seed_stream") \
    X(AUD_HOIST, "DSH_AUD_HOIST", INT, "1", PROCESS, AB_EXACT, "encoder_aud's timestep-independent front once per condition; 0 in every evaluation") \
    X(AUD_FUSE, "DSH_AUD_FUSE", INT, "1", CALL, AB_ROUNDOFF, "encoder_aud's tail as one launch; 0 six launches") \
    X(APROJ_TL, "DSH_APROJ_TL", INT, "1", CALL, AB_ROUNDOFF, "audio_proj of both encoders as one token-per-lane launch; 0 two (GEMM + tile_rows)") \
    X(GEMM_KSPLIT, "DSH_GEMM_KSPLIT", INT, "512", PROCESS, PRODUCT, "fp32: row limit of the few-row K-split GEMM (0 off: the reproducible mode).  Latched in gemm.hip; the denoiser reads it afresh per CONTEXT for where its fused launches take over, so changing it inside a process leaves the two disagreeing") \
    X(GEMV, "DSH_GEMV", INT, "1", PROCESS, AB_ROUNDOFF, "Linears of at most 16 rows on the weight-streaming GEMV; 0 the tiled GEMM (one latch for the fp32 and the bf16 launcher, which used to latch each at its own first launch)") \
    X(GEMM_VARIANT, "DSH_GEMM_VARIANT", INT, "1", PROCESS, BENCH, "GEMM main-loop variant (kernel bench hook; one latch for both launchers, as DSH_GEMV)") \
    X(GEMM_TILE, "DSH_GEMM_TILE", INT, "1", PROCESS, AB_ROUNDOFF, "GEMM tile shape: 0 always 128 x 128, 2 / 3 / 4 always 128 x 64 / 64 x 64 / 64 x 32 (one latch for both launchers, as DSH_GEMV)") \
    X(GP_DMA, "DSH_GP_DMA", INT, "1", PROCESS, AB_EXACT, "fp32: operands of the gemm_f32_pro.hip launches by LDS-DMA; 0 through registers") \
    X(GP_ABL, "DSH_GP_ABL", INT, "0", PROCESS, BENCH, "fp32 GEMM launches drop parts of their main loop (results are garbage; warns)") \
    X(ATTN_F32_MFMA, "DSH_ATTN_F32_MFMA", INT, "1", PROCESS, AB_ROUNDOFF, "fp32, 64-channel heads: attention on the exact-fp32 matrix pipe; 0 the VALU kernels") \
    X(ATTN_STY, "DSH_ATTN_STY", INT, "1", PROCESS, AB_ROUNDOFF, "fp32: the attention branch's StylizationBlock front inside the attention launch (windows up to 64 frames); 0 two launches") \
    X(F32_FUSE, "DSH_F32_FUSE", INT, "15", CONTEXT, AB_ROUNDOFF, "fp32 D = 512 model only (& 15): 1 folded LayerNorms, 2 StylizationBlock fronts, 4 front-less Linears on the pipelined loop, 8 front inside attention; 0 the row kernels") \
    X(TL_RAW, "DSH_TL_RAW", INT, "0", CALL, BENCH, "dsh_op_tl_linear passes every operand through untouched (timing loops)") \
    X(TL_DBG, "DSH_TL_DBG", INT, "0", CALL, BENCH, "dsh_op_tl_linear: the kernel's dbg argument (ablations)") \
    X(TL_CLK, "DSH_TL_CLK", INT, "0", CALL, BENCH, "dsh_op_tl_linear: clock probe of block 0 in per-call scratch, so every value synchronises before return; 2 also reads it back and prints") \
    X(TL_TRACE, "DSH_TL_TRACE", STR, "unset", CALL, BENCH, "file name: block timeline of a dsh_op_tl_linear / dsh_op_tl2_ffn call (synchronises)") \
    X(TL_PROBE, "DSH_TL_PROBE", STR, "unset", CALL, BENCH, "file name: per-block phase probe of the second-generation kernels (synchronises)")

enum Switch : int {
#define DSH_SWITCH_ID(id, name, kind, def, when, cls, help) SW_##id,
    DSH_SWITCH_TABLE(DSH_SWITCH_ID)
#undef DSH_SWITCH_ID
    SW_COUNT
};

struct SwitchInfo {
    const char* name; SwitchKind kind; const char* def; long def_int; SwitchWhen when; SwitchClass cls; const char* help;
};
// leading integer of a default's text ("21500 (fp32: 2900)" -> 21500, "unset" -> 0)
constexpr long switch_default_int(const char* s) { long v = 0; for (; *s >= '0' && *s <= '9'; ++s) v = v * 10 + (*s - '0'); return v; }
constexpr bool switch_name_is(const char* name, const char* id) {      // name == "DSH_" id
    for (const char* p = "DSH_"; *p; ++p, ++name) if (*name != *p) return false;
    for (; *id; ++id, ++name) if (*name != *id) return false;
    return *name == 0;
}
inline constexpr SwitchInfo kSwitches[SW_COUNT] = {
#define DSH_SWITCH_ROW(id, name, kind, def, when, cls, help) {name, SWK_##kind, def, switch_default_int(def), SWW_##when, SWC_##cls, help},
    DSH_SWITCH_TABLE(DSH_SWITCH_ROW)
#undef DSH_SWITCH_ROW
};
#define DSH_SWITCH_CHECK(id, name, kind, def, when, cls, help) static_assert(switch_name_is(name, #id), "switch id and variable name differ: " name);
DSH_SWITCH_TABLE(DSH_SWITCH_CHECK)
#undef DSH_SWITCH_CHECK

// ---- accessors ---------------------------------------------------------------------------------------------------------------------
struct SwitchValue {
    bool set;           // the variable is present in the environment
    long v;             // atoi of its text (0 when unset)
    const char* text;   // its text, null when unset
};
inline SwitchValue switch_read_now(Switch id) {      // one environment lookup, whatever the entry's `when`
    const char* e = getenv(kSwitches[id].name);
    return {e != nullptr, e ? atol(e) : 0, e};
}
inline const SwitchValue& switch_latched(Switch id) {
    struct Slot { std::atomic<bool> ready{false}; SwitchValue val{false, 0, nullptr}; std::string text; };
    static Slot slots[SW_COUNT];
    static std::mutex mu;
    Slot& s = slots[id];
    if (!s.ready.load(std::memory_order_acquire)) {
        std::lock_guard<std::mutex> lock(mu);
        if (!s.ready.load(std::memory_order_relaxed)) {
            s.val = switch_read_now(id);
            if (s.val.text) { s.text = s.val.text; s.val.text = s.text.c_str(); }      // (the environment may change under the latch)
            s.ready.store(true, std::memory_order_release);
        }
    }
    return s.val;
}
// as the entry says: the latched value of a PROCESS switch, a fresh read of every other
inline SwitchValue switch_value(Switch id) { return kSwitches[id].when == SWW_PROCESS ? switch_latched(id) : switch_read_now(id); }

inline bool switch_get(Switch id, long* v) { const SwitchValue s = switch_value(id); if (s.set) *v = s.v; return s.set; }   // is it set, and to what integer
inline long switch_int(Switch id) { const SwitchValue s = switch_value(id); return s.set ? s.v : kSwitches[id].def_int; }    // integer, or the entry's default
inline bool switch_present(Switch id) { return switch_value(id).set; }
inline const char* switch_str(Switch id) { return switch_value(id).text; }                                                    // text, or null
// the second readers of a PROCESS switch that look again (see the entry)
inline long switch_int_now(Switch id) { const SwitchValue s = switch_read_now(id); return s.set ? s.v : kSwitches[id].def_int; }
inline bool switch_present_now(Switch id) { return switch_read_now(id).set; }
// "overrides only when positive": the value when it is set and > 0, else 0
inline long switch_positive(Switch id) { const SwitchValue s = switch_value(id); return s.set && s.v > 0 ? s.v : 0; }

// ---- derivations shared by more than one reader (or with a quirk worth one statement) ------------------------------------------------
// sub-batch streams: unset 3; "0" -> 1 stream, "1" -> 2, n -> n, clamped to 1 .. 8
inline int dual_streams() {
    long v = 0;
    if (!switch_get(SW_DUAL, &v)) return (int)kSwitches[SW_DUAL].def_int;
    return v == 0 ? 1 : (int)std::max(1L, std::min(8L, v == 1 ? 2L : v));
}
// fused-FFN kernel generation (denoiser, dsh_op_tl2_ffn, profiler.h): only 2 selects generation 2
inline int ffn_generation() { return switch_int(SW_FFN_V) == 2 ? 2 : 3; }
// fused-FFN variants (tl3_ffn.hip launches by them, the denoiser counts the bytes they move)
inline int ffn_pc() { return (int)std::min(2L, std::max(0L, switch_int(SW_FFN_PC))); }
inline int ffn_pb() { return (int)(switch_int(SW_FFN_PB) & 3); }
inline bool ffn_keeps_hi_plane() { return (ffn_pb() & 1) && ffn_pc() == 1; }
// fp32 few-row GEMM: launches of at most this many rows take it (gemm.hip, latched); the denoiser's fused fp32 launches start above
// the value its context read at construction
inline int gemm_ksplit_rows() { return (int)switch_int(SW_GEMM_KSPLIT); }
inline int gemm_ksplit_rows_context() { return (int)switch_int_now(SW_GEMM_KSPLIT); }
// loops of at most this many token rows run as one batch on two encoder streams (sampler, latched; DenoiserContext per context)
inline size_t pipe_rows() { return (size_t)switch_int(SW_PIPE_ROWS); }
inline size_t pipe_rows_context() { return (size_t)switch_int_now(SW_PIPE_ROWS); }
// the pipelined loop restores every head from the slots a side-stream prefetch run fills: all three must be on
inline bool pipe_switches_on() { return switch_int(SW_PIPE) != 0 && switch_int(SW_LEVEL_PREFETCH) != 0 && switch_int(SW_LEVEL_CACHE) != 0; }
// The two meanings of an unset DSH_HILO.  In the denoiser the planes are the product default, so unset is ON and only 0 switches them
// off.  The op entries (dsh_op_tl_linear, dsh_op_tl2_ffn) are test helpers: a plain call runs the fp32-residual instantiation, and a
// test asks for the plane instantiation explicitly, so unset is OFF and only a non-zero value switches it on.
inline bool hilo_denoiser() { long v = 0; return !(switch_get(SW_HILO, &v) && v == 0); }
inline bool hilo_op() { long v = 0; return switch_get(SW_HILO, &v) && v != 0; }
inline int f32_fuse_bits() { return (int)(switch_int(SW_F32_FUSE) & 15); }

// what dsh_switch_read answers for a derivation's name (tests pin the parsing quirks through these)
struct SwitchDerived { const char* name; long (*fn)(); };
inline constexpr SwitchDerived kSwitchDerived[] = {
    {"dual_streams", [] { return (long)dual_streams(); }},
    {"ffn_generation", [] { return (long)ffn_generation(); }},
    {"ffn_pc", [] { return (long)ffn_pc(); }},
    {"ffn_pb", [] { return (long)ffn_pb(); }},
    {"ffn_keeps_hi_plane", [] { return (long)ffn_keeps_hi_plane(); }},
    {"gemm_ksplit_rows", [] { return (long)gemm_ksplit_rows(); }},
    {"gemm_ksplit_rows_context", [] { return (long)gemm_ksplit_rows_context(); }},
    {"pipe_rows", [] { return (long)pipe_rows(); }},
    {"pipe_rows_context", [] { return (long)pipe_rows_context(); }},
    {"pipe_switches_on", [] { return (long)pipe_switches_on(); }},
    {"hilo_denoiser", [] { return (long)hilo_denoiser(); }},
    {"hilo_op", [] { return (long)hilo_op(); }},
    {"f32_fuse_bits", [] { return (long)f32_fuse_bits(); }},
    {"tls_rows_override", [] { return switch_positive(SW_TLS_ROWS); }},      // (switch_positive, through one of its three users)
};

}  // namespace dsh
