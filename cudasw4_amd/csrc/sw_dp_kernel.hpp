// sw_dp_kernel.hpp — the Smith-Waterman DP-matrix fill for gfx950 (MI355X), all four arithmetic kinds.
//
// Replaces the reference's NW_local_affine_{single,multi}_pass_{half2,dpx_s16,dpx_s32,float}
// kernels (half2_kernels.cuh:798-1125, dpx_s16_kernels.cuh:765-1056, dpx_s32_kernels.cuh:777-1017,
// float_kernels.cuh:788-1023).  NOT a translation: the reference keeps the SUBJECT in registers and
// streams the query through a 32-lane warp with a 37 KB pair table gathered from shared memory.
// Here the orientation is transposed and built around CDNA4's DPP rows:
//
//   * one alignment group == one DPP row of 16 lanes; a wave64 runs 4 independent groups (for the few long
//     subjects of a real DB: group == the whole wave, 64 lanes, wave_shr:1);
//   * the QUERY is tiled in stripes of LANES*R rows; lane l of a group owns R consecutive query rows
//     and keeps their H (previous column) and E (horizontal gap) state in VGPRs;
//   * subject letters stream through the row: at step t lane l works on subject column t-l
//     (anti-diagonal wavefront).  H and F of a lane's bottom row go to lane l+1 with
//     v_mov_b32_dpp row_shr:1 (lane 0 is fed by bound_ctrl zero-fill or by the previous stripe);
//   * the substitution scores come from a per-query PROFILE tile in LDS: for subject letter c the
//     lane reads its R scores as contiguous 16-byte chunks (ds_read_b128), laid out so that the
//     bank of an access depends on the lane only -> conflict-free for any mix of letters;
//   * packed kinds run two subjects per group in the two 16-bit halves (v_pk_add_f16 / v_pk_maximum3_f16; the int16
//     kind adds with v_pk_add_u16 / v_pk_sub_u16 and compares its biased bit patterns with the same fp16 maximum);
//     with 16-lane groups their profile entries are WIDE words (score, 1), so that one v_pk_fma_f16 / v_pk_mad_u16
//     with op_sel pairs the two subjects' scores AND adds them to the diagonal (Arith::add_pair);
//   * the recurrence runs in a column-offset frame (dp_step<OFFS>): every value of subject column j is kept raised by
//     |gex| * (j mod K + LANES), which takes the "+ gex" out of the horizontal gap state, and lane-local row r by a
//     further |gex| * (r mod P) (row classes), which takes it out of the vertical gap state except where the class
//     wraps: 5.8 instead of 8.5 instructions per cell pair; the plain form remains in the 32-bit kinds only, for
//     gap-extension scores too large for any K (a packed launch that cannot run the column-offset form is served by its
//     32-bit kind: sw_launch.hpp).  The packed sw_scan_kernel runs it in the UNIFORM frame instead: a cell of step t of stripe s is
//     raised by |gex| * ((t + LANES*s) mod K + 1 + class), the same zero levels in every lane of the wave — held in scalar
//     registers, the frame lowered by every lane in the same step (sw_scan_kernel explains the constants); the streamed
//     kernels keep the column frame;
//   * queries longer than one stripe are processed stripe after stripe by the same group; the H/F
//     row at the stripe border is spilled to a small global scratch (branch-free: 8 bytes stored per
//     step, 32 bytes loaded per four steps), the analogue of the reference's devTempHcol2/devTempEcol2;
//   * persistent workgroups pull batches of groups from an atomic counter, longest subjects first.
//
// Padding is self-neutralising exactly as in the reference: query rows >= Q and
// subject columns >= len use letter code 20 whose scores are all negative.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sw_pssm.hpp"

namespace swk {

typedef uint32_t u32;
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr int kGroup = 16;        // lanes per alignment group in the standard shape (one DPP row)
constexpr int kThreads = 256;     // workgroup size: 4 waves = 16 row groups or 4 wave-wide groups
constexpr int kPadLetter = 20;    // code used for padding rows / columns
constexpr int kLetters = 21;

enum { F16X2 = 0, I16X2 = 1, I32 = 2, F32 = 3 };

// DPP controls (GFX9 encoding)
constexpr int DPP_ROW_SHL1 = 0x101;   // lane i <- lane i+1 (within a row of 16)
constexpr int DPP_ROW_SHR1 = 0x111;   // lane i <- lane i-1
constexpr int DPP_ROW_ROR1 = 0x121;
constexpr int DPP_QUAD_SHR1 = 0x90;   // quad_perm [0,0,1,2]: lane i <- lane i-1 within its quad (lane 0 of a quad: itself)
constexpr int DPP_WAVE_SHL1 = 0x130;  // the same across all 64 lanes of the wave
constexpr int DPP_WAVE_SHR1 = 0x138;

// The group shape: LANES = 16 (one DPP row per alignment group, 4 groups per wave: the bulk of a DB),
// LANES = 64 (the whole wave is one anti-diagonal pipeline: long subjects, 4x the lanes per alignment so
// that the few giant sequences of a real DB do not become the tail of the scan), or
// LANES = 8 (half a DPP row, 8 groups per wave: SHORT QUERIES.  A query of Q rows gives every lane Q/8 instead of Q/16
// rows, so the per-step work that does not scale with the rows (lane exchange, letter handling, window upkeep: ~10
// instructions) is spread over twice the cells, and the pipeline fill per subject is 7 instead of 15 steps.  The
// row_shr:1 exchange crosses from lane 7 into lane 8, the head of the second group of the row, which costs one select
// per exchanged value (prev_lane).  With several stripes the shape pays off for short subjects only: half the fill per
// stripe, but twice the stripes.), or
// LANES = 4 (a DPP quad, 16 groups per wave: VERY SHORT QUERIES, single-stripe only.  A 48-residue query gives an 8-lane
// group 6 rows per lane — (6.5 * 6 + 19) / 6 = 9.67 instructions per cell pair, SQ_INSTS_VALU says the same — and a quad 12:
// 8.08.  The exchange is a quad_perm, every group's head selects its boundary value like lane 8 above.)
template <int LANES>
struct Shift {
    static_assert(LANES == 4 || LANES == 8 || LANES == 16 || LANES == 64, "group = a DPP quad, half a DPP row, a DPP row or the whole wave");
    static constexpr int kShr1 = LANES <= 16 ? DPP_ROW_SHR1 : DPP_WAVE_SHR1;
    static constexpr int kShl1 = LANES <= 16 ? DPP_ROW_SHL1 : DPP_WAVE_SHL1;
};

template <int CTRL, bool ZERO_FILL>
__device__ __forceinline__ u32 dpp(u32 old, u32 src) {
    return (u32)__builtin_amdgcn_update_dpp((int)old, (int)src, CTRL, 0xf, 0xf, ZERO_FILL);
}

// The value of the previous lane of the group; the group's head lane takes `headval` (ZERO_FILL: headval must be 0 and
// the head is filled by bound_ctrl).  8-lane groups: lane 8 of a DPP row is a head too but has a source lane, so it
// is selected explicitly (`head` is loop-invariant: one v_cndmask with an SGPR mask).
template <int LANES, bool ZERO_FILL>
__device__ __forceinline__ u32 prev_lane(u32 headval, u32 src, bool head) {
    if constexpr (LANES == 8) {
        const u32 v = dpp<DPP_ROW_SHR1, false>(headval, src);
        return head ? headval : v;
    } else if constexpr (LANES == 4) {
        const u32 v = dpp<DPP_QUAD_SHR1, false>(headval, src);
        return head ? headval : v;
    } else {
        (void)head;
        return dpp<Shift<LANES>::kShr1, ZERO_FILL>(headval, src);
    }
}

// ------------------------------------------------------------------------------------------------
// Arithmetic traits.  All state lives in 32-bit registers; E and F are kept CLAMPED at zero
// (E' = max(E,0), F' = max(F,0)), which leaves H = max(diag+s, E', F') unchanged and makes the
// explicit max(.,0) of the reference recurrence (half2_kernels.cuh:176) free.
// ------------------------------------------------------------------------------------------------
template <int KIND>
struct Arith;

// int16 kind.  State is kept BIASED by 1024 in unsigned 16-bit fields: H~ = H + 1024, E~ = E' + 1024, F~ likewise.
// Adds/subtracts are integer (v_pk_add_u16 / v_pk_sub_u16); every maximum is taken with the fp16 comparator
// v_pk_maximum3_f16 ON THE INTEGER BIT PATTERNS: for patterns in [0x0400, 0x7BFF] (positive normal halves) the
// fp16 order equals the integer order and the instruction returns one of its inputs bit-exactly, so the
// 3-input maximum the int16 ISA lacks comes for free (8.5 instead of 10 instructions per cell pair).
//   * diag+s can dip below 1024 (a denormal pattern, possibly flushed): it then loses against E~ >= 1024
//     anyway, so the result is unaffected;
//   * patterns >= 0x7C00 (inf/NaN, H >= 30720) only arise after the running maximum has passed the
//     25000 overflow limit (H grows by at most max(s) per anti-diagonal), and a NaN maximum is itself
//     >= the limit, so such subjects are always flagged and re-scored in 32 bits.
template <>
struct Arith<I16X2> {
    static constexpr bool kPacked = true;
    static constexpr int kSubjects = 2;
    static constexpr int kLimit = 25000;  // kernels.cuh:5 MAX_ACC_SHORT
    static constexpr bool kWindow = true;  // StripeState: zero levels and maxima as windows over a quad
    static constexpr int kBias = 1024;
    static constexpr u32 kZero = (u32)kBias | ((u32)kBias << 16);  // the value 0 in both halves
    // gap scores are <= 0; magnitudes are subtracted (|g| <= 1000 keeps E~ - |g| non-negative)
    static __host__ __device__ u32 encode_gap(int g) { u32 m = (u32)(-g) & 0xffffu; return m | (m << 16); }
    static __host__ __device__ u32 encode_score(int s) { return (u32)(uint16_t)(int16_t)s; }
    static __device__ __forceinline__ u32 add(u32 a, u32 b) {
        return __builtin_bit_cast(u32, (u16x2)(__builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b)));
    }
    static __device__ __forceinline__ u32 max3(u32 a, u32 b, u32 c) {
        return __builtin_bit_cast(u32, __builtin_elementwise_maximum(
            __builtin_elementwise_maximum(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b)),
            __builtin_bit_cast(f16x2, c)));
    }
    static __device__ __forceinline__ u32 max2(u32 a, u32 b) {
        return __builtin_bit_cast(u32, __builtin_elementwise_maximum(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b)));
    }
    static __device__ __forceinline__ u32 cell_h(u32 t, u32 e, u32 f) { return max3(t, e, f); }
    static __device__ __forceinline__ u32 gap(u32 a, u32 g) {
        return __builtin_bit_cast(u32, (u16x2)(__builtin_bit_cast(u16x2, a) - __builtin_bit_cast(u16x2, g)));
    }
    static __device__ __forceinline__ u32 fold2(u32 m, u32 a, u32 b) { return max3(m, a, b); }
    // column-offset recurrence (dp_step<OFFS>): the zero level of column offset k, +a, star -> true values
    static __host__ __device__ u32 zero_at(int a, int k) { u32 z = (u32)(kBias + a * k) & 0xffffu; return z | (z << 16); }
    static __host__ __device__ u32 pos_word(int a) { u32 m = (u32)a & 0xffffu; return m | (m << 16); }
    // the zero level v (sw_stream_kernel.hpp: levels with a base and jumps) in both halves
    static __device__ __forceinline__ u32 level_word(int v) { const u32 z = (u32)(kBias + v) & 0xffffu; return z | (z << 16); }
    static __device__ __forceinline__ u32 true_of(u32 m, u32 z) { return gap(m, z); }  // plain unsigned integers
    // frame lowering by the magnitude word w (saturating: see sw_scan_kernel's lower_frame for the one value it can reach)
    static __device__ __forceinline__ u32 lower(u32 a, u32 w) {
        return __builtin_bit_cast(u32, __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, w)));
    }
    static __device__ __forceinline__ u32 true_max(u32 a, u32 b) {
        return __builtin_bit_cast(u32, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
    }
    static __device__ __forceinline__ int true_lo(u32 v) { return (int)(v & 0xffffu); }
    static __device__ __forceinline__ int true_hi(u32 v) { return (int)(v >> 16); }
    // wide profile words (score, 1): (wa.lo * wb.hi + c.lo, wa.hi * wb.lo + c.hi) = c + (score A, score B) in ONE
    // v_pk_mad_u16 (op_sel swaps the halves of wb) — replaces the v_perm_b32 + add of the two-rows-per-word layout
    static constexpr u32 kOne = 1u;
    static __device__ __forceinline__ u32 add_pair(u32 wa, u32 wb, u32 c) {
        u32 d;
        asm("v_pk_mad_u16 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(wa), "v"(wb), "v"(c));
        return d;
    }
};

template <>
struct Arith<F16X2> {
    static constexpr bool kPacked = true;
    static constexpr int kSubjects = 2;
    static constexpr int kLimit = 2048;  // kernels.cuh:4 MAX_ACC_HALF2
    static constexpr bool kWindow = true;
    static constexpr u32 kZero = 0u;
    static __host__ __device__ u32 half_bits(int v) {
        // exact conversion of a small integer |v| < 2048 to IEEE binary16 bits
        if (v == 0) return 0;
        u32 sign = v < 0 ? 0x8000u : 0u;
        u32 a = (u32)(v < 0 ? -v : v);
        int e = 0;
        while ((a >> (e + 1)) != 0) e++;
        u32 mant = (a << (10 - e)) & 0x3ffu;
        return sign | ((u32)(e + 15) << 10) | mant;
    }
    static __host__ __device__ u32 encode_gap(int g) { u32 h = half_bits(g); return h | (h << 16); }
    static __host__ __device__ u32 encode_score(int s) { return half_bits(s); }
    static __device__ __forceinline__ u32 add(u32 a, u32 b) {
        return __builtin_bit_cast(u32, (f16x2)(__builtin_bit_cast(f16x2, a) + __builtin_bit_cast(f16x2, b)));
    }
    static __device__ __forceinline__ u32 max3(u32 a, u32 b, u32 c) {
        return __builtin_bit_cast(u32, __builtin_elementwise_maximum(
            __builtin_elementwise_maximum(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b)),
            __builtin_bit_cast(f16x2, c)));
    }
    static __device__ __forceinline__ u32 max2(u32 a, u32 b) {
        return __builtin_bit_cast(u32, __builtin_elementwise_maximum(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b)));
    }
    static __device__ __forceinline__ u32 cell_h(u32 t, u32 e, u32 f) { return max3(t, e, f); }
    static __device__ __forceinline__ u32 gap(u32 a, u32 g) { return add(a, g); }  // not clamped yet
    static __device__ __forceinline__ u32 fold2(u32 m, u32 a, u32 b) { return max3(m, a, b); }  // one v_pk_maximum3_f16 per two rows
    static __host__ __device__ u32 zero_at(int a, int k) { u32 h = half_bits(a * k); return h | (h << 16); }
    static __host__ __device__ u32 pos_word(int a) { u32 h = half_bits(a); return h | (h << 16); }
    // the zero level v (|v| <= 2048: exact) in both halves, by the hardware conversion
    static __device__ __forceinline__ u32 level_word(int v) {
        const u32 h = (u32)__builtin_bit_cast(unsigned short, (_Float16)(float)v);
        return h | (h << 16);
    }
    static __device__ __forceinline__ u32 true_of(u32 m, u32 z) {
        return __builtin_bit_cast(u32, (f16x2)(__builtin_bit_cast(f16x2, m) - __builtin_bit_cast(f16x2, z)));
    }
    static __device__ __forceinline__ u32 lower(u32 a, u32 w) { return add(a, w); }  // w = encode_gap(-a*K)
    static __device__ __forceinline__ u32 true_max(u32 a, u32 b) { return max2(a, b); }
    static __device__ __forceinline__ int true_lo(u32 v) { return (int)(float)__builtin_bit_cast(f16x2, v).x; }
    static __device__ __forceinline__ int true_hi(u32 v) { return (int)(float)__builtin_bit_cast(f16x2, v).y; }
    // wide profile words (score, 1.0): one v_pk_fma_f16 with op_sel (exact: a product with 1.0, one rounding of an integer sum)
    static constexpr u32 kOne = 0x3c00u;
    static __device__ __forceinline__ u32 add_pair(u32 wa, u32 wb, u32 c) {
        // spelled out: from a shufflevector hipcc folds the swap into op_sel for three words of a 16-byte LDS chunk but
        // rotates the first one with an extra v_alignbit_b32
        u32 d;
        asm("v_pk_fma_f16 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(wa), "v"(wb), "v"(c));
        return d;
    }
};

template <>
struct Arith<I32> {
    static constexpr bool kPacked = false;
    static constexpr int kSubjects = 1;
    static constexpr int kLimit = 0x7fffffff;
    static constexpr bool kWindow = true;
    static constexpr u32 kZero = 0u;
    static __host__ __device__ u32 encode_gap(int g) { return (u32)g; }
    static __host__ __device__ u32 encode_score(int s) { return (u32)s; }
    // v_max3_i32 spelled out: hipcc's own selection mixes signed/unsigned 2- and 3-input forms here
    // (4.4 max instructions per cell instead of 3.5).  The compiler puts a wait state behind each inline-asm result that
    // is read at once; the plain-C++ form has none but spills more under the occupancy bound (5.6 vs 6.0 TCUPS)
    static __device__ __forceinline__ u32 max3(u32 a, u32 b, u32 c) {
        u32 d;
        asm("v_max3_i32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
        return d;
    }
    static __device__ __forceinline__ u32 max3_zero(u32 a, u32 b) {
        u32 d;
        asm("v_max3_i32 %0, %1, %2, 0" : "=v"(d) : "v"(a), "v"(b));
        return d;
    }
    static __device__ __forceinline__ u32 add(u32 a, u32 b) { return a + b; }
    static __device__ __forceinline__ u32 max2(u32 a, u32 b) { return (u32)((int)a > (int)b ? (int)a : (int)b); }
    static __device__ __forceinline__ u32 cell_h(u32 t, u32 e, u32 f) { return max3(t, e, f); }
    static __device__ __forceinline__ u32 gap(u32 a, u32 g) { return a + g; }
    static __device__ __forceinline__ u32 gap_state(u32 ext, u32 open) { return max3_zero(ext, open); }
    static __device__ __forceinline__ u32 fold2(u32 m, u32 a, u32 b) { return max3(m, a, b); }
    static __device__ __forceinline__ int score_lo(u32 v) { return (int)v; }
    static __host__ __device__ u32 zero_at(int a, int k) { return (u32)(a * k); }
    static __host__ __device__ u32 pos_word(int a) { return (u32)a; }
    static __device__ __forceinline__ u32 true_of(u32 m, u32 z) { return m - z; }
    static __device__ __forceinline__ u32 true_max(u32 a, u32 b) { return max2(a, b); }
    static __device__ __forceinline__ int true_lo(u32 v) { return (int)v; }
    static __device__ __forceinline__ int true_hi(u32) { return 0; }
};

template <>
struct Arith<F32> {
    static constexpr bool kPacked = false;
    static constexpr int kSubjects = 1;
    static constexpr int kLimit = 0x7fffffff;
    // the fp32 kernels (168 VGPRs for three waves per SIMD) spill in their loops with the 7 extra window registers
    // (7.9 -> 1.6 TCUPS): they add a per step to P zero levels and P maxima instead
    static constexpr bool kWindow = false;
    static constexpr u32 kZero = 0u;
    static __host__ __device__ u32 encode_gap(int g) { return __builtin_bit_cast(u32, (float)g); }
    static __host__ __device__ u32 encode_score(int s) { return __builtin_bit_cast(u32, (float)s); }
    static __device__ __forceinline__ float f(u32 v) { return __builtin_bit_cast(float, v); }
    static __device__ __forceinline__ u32 u(float v) { return __builtin_bit_cast(u32, v); }
    static __device__ __forceinline__ u32 add(u32 a, u32 b) { return u(f(a) + f(b)); }
    static __device__ __forceinline__ u32 max2(u32 a, u32 b) { return u(__builtin_fmaxf(f(a), f(b))); }
    static __device__ __forceinline__ u32 max3(u32 a, u32 b, u32 c) { return u(__builtin_fmaxf(__builtin_fmaxf(f(a), f(b)), f(c))); }
    static __device__ __forceinline__ u32 cell_h(u32 t, u32 e, u32 ff) { return u(__builtin_fmaxf(__builtin_fmaxf(f(t), f(e)), f(ff))); }
    static __device__ __forceinline__ u32 gap(u32 a, u32 g) { return u(f(a) + f(g)); }
    static __device__ __forceinline__ u32 gap_state(u32 ext, u32 open) { return u(__builtin_fmaxf(__builtin_fmaxf(f(ext), f(open)), 0.0f)); }
    static __device__ __forceinline__ u32 fold2(u32 m, u32 a, u32 b) { return u(__builtin_fmaxf(__builtin_fmaxf(f(m), f(a)), f(b))); }  // v_max3_f32
    static __device__ __forceinline__ int score_lo(u32 v) { return (int)f(v); }
    static __host__ __device__ u32 zero_at(int a, int k) { return __builtin_bit_cast(u32, (float)(a * k)); }
    static __host__ __device__ u32 pos_word(int a) { return __builtin_bit_cast(u32, (float)a); }
    static __device__ __forceinline__ u32 true_of(u32 m, u32 z) { return u(f(m) - f(z)); }
    static __device__ __forceinline__ u32 true_max(u32 a, u32 b) { return max2(a, b); }
    static __device__ __forceinline__ int true_lo(u32 v) { return (int)f(v); }
    static __device__ __forceinline__ int true_hi(u32) { return 0; }
};

// ------------------------------------------------------------------------------------------------
// Profile tile geometry (shared by the profile builder and the kernel).
//   NW     32-bit words a lane reads per letter per step (ceil(R/2) packed, R scalar)
//   NCH    16-byte chunks per lane per letter
//   letter row  = NCH chunks-rows of 256 bytes: chunk k of lane l at  k*256 + l*16
//   tile        = 21 letter rows, preceded by 16 bytes (lane addresses carry a +16 bias, see Step)
// ------------------------------------------------------------------------------------------------
// How the NW words a lane reads per letter are cut into 16-byte LDS slots ("chunks").  LDS serves ds_read_b128 and
// ds_read_b96 of this layout (one 16-byte slot per lane, letter rows a multiple of 256 bytes apart) without bank
// conflicts for ANY mix of letter rows across the groups of a wave, but not ds_read_b32 / ds_read_b64: those are
// processed 64 / 32 lanes at a time, and the lanes of different groups then meet in the same banks at different
// addresses (measured on ragged subjects, where the groups read different letters: 11-37 % of the LDS cycles of the
// NW mod 4 = 1 kernels were conflicts, 4-12 % for NW mod 4 = 2; the identical subjects of the peak DB hid it).  So a
// word count that is no multiple of 4 is cut into 4-word chunks and one to three 3-WORD chunks (42 = 9 x 4 + 2 x 3,
// 45 = 9 x 4 + 3 x 3, 43 = 10 x 4 + 3): the same number of reads and of LDS bytes as full chunks plus a short tail, no
// register holds a word nobody needs (reading the short tail as b96 and dropping a word cost 2.5 % in the 256-VGPR
// kernels), and every read is conflict-free.  NW = 1, 2, 5 cannot be cut that way: their tail is a b96 read of which
// one or two words are used.
template <int NW>
struct Chunks {
    static constexpr int kRem = NW % 4;
    static constexpr int kWant3 = (4 - kRem) % 4;
    static constexpr bool kSplit = NW >= 3 * kWant3;
    static constexpr int kN3 = kSplit ? kWant3 : 1;                      // 3-word chunks (not kSplit: ONE partly used one)
    static constexpr int kN4 = kSplit ? (NW - 3 * kWant3) / 4 : NW / 4;  // 4-word chunks, in front
    static constexpr int kCount = kN4 + kN3;
    static constexpr int first(int c) { return c < kN4 ? 4 * c : 4 * kN4 + 3 * (c - kN4); }  // first word of chunk c
    static constexpr int words(int c) { return c < kN4 ? 4 : (kSplit ? 3 : kRem); }            // words of chunk c in use
    static constexpr int chunk_of(int w) { return w < 4 * kN4 ? w / 4 : kN4 + (w - 4 * kN4) / 3; }
    static constexpr bool starts_chunk(int w) { return first(chunk_of(w)) == w; }
    // progressive reads: `lead` chunks are issued at the top of a step, chunk c + lead when the chain reaches the first
    // word of chunk c; a word that is consumed `ahead` words before the chain reaches it must have been issued at least
    // `slack` rows earlier (the LDS latency hides behind them)
    static constexpr bool lead_ok(int lead, int ahead, int slack) {
        for (int r = 0; r < NW; r++) {
            const int need = chunk_of(r + ahead < NW ? r + ahead : NW - 1);
            if (need >= lead && first(need - lead) + slack > r) return false;
        }
        return true;
    }
    static constexpr int lead_for(int ahead, int slack) {
        int lead = 1;
        while (lead < kCount && !lead_ok(lead, ahead, slack)) lead++;
        return lead;
    }
};

template <int KIND, int R, int LANES = kGroup>
struct Geometry {
    static constexpr bool kPacked = Arith<KIND>::kPacked;
    // packed kinds, 16-lane groups: WIDE words (score of the row, 1) — the pair (score A, score B) of a cell pair and its
    // addition to the diagonal are ONE packed multiply-add (Arith::add_pair).  Wave-wide groups keep two query rows per
    // word (an odd R leaves the upper half of the last word unused) and pair the scores with v_perm_b32.
    static constexpr bool kWide = kPacked && LANES <= 16;
    static constexpr int NW = (kPacked && !kWide) ? (R + 1) / 2 : R;
    using C = Chunks<NW>;
    static constexpr int NCH = C::kCount;
    // chunk k of lane l at k*kChunkRowBytes + l*16; 8-lane groups keep the 16 slots of a DPP row: the first group of a row
    // reads slots 0..7, the second one slots 8..15 (dp_step: laneStep), which the profile builder fills with a copy —
    // sharing slots 0..7 made the two groups meet in the same banks with different letter rows
    static constexpr int kChunkRowBytes = (LANES <= 16 ? 16 : LANES) * 16;
    static constexpr int kRowBytes = NCH * kChunkRowBytes;
    static constexpr int kTileBytes = kLetters * kRowBytes;
    static constexpr int kStripeRows = LANES * R;
    // a letter travels as (letter * kLetterUnits) in one byte; its row offset is that byte << kLetterShift
    static constexpr int kLetterShift = LANES <= 16 ? 8 : 10;
    static constexpr int kLetterUnits = kRowBytes >> kLetterShift;
    static_assert(kPadLetter * kLetterUnits < 256, "letter offset must fit a byte");
};

// Uniform frame (packed sw_scan_kernel: ScanParams::uniform_frame): longest frame period and the entries of the level table
constexpr int kUniformMaxPeriod = 256;
constexpr int kLevelWords = kUniformMaxPeriod + 16;

struct ScanParams {
    const int8_t* chars;
    const uint64_t* offsets;
    const int32_t* lengths;
    const int32_t* positions;  // optional indirection list (overflow re-score); nullptr -> first_pos + i
    const int32_t* count_ptr;  // optional device-side count; nullptr -> n
    int32_t first_pos;
    int32_t n;
    const unsigned char* profile;  // nstripes tiles of Geometry::kTileBytes
    int32_t nstripes;
    u32 gop, gex;              // Arith<KIND>::encode_gap
    float* scores;
    int32_t* ids;
    int64_t id_offset;
    int32_t* ovf_pos;
    int32_t* ovf_count;
    int32_t ovf_check;
    u32* scratch;              // stripe-border spill and address stream: per (workgroup, group) group_region_words(lcap) words
    int32_t lcap;
    int32_t len_bound;         // the caller's max_subject_len rounded up to whole letter words (a multiple of 4): multi-stripe kernels take a longer subject's first len_bound residues (lcap is sized from it)
    const u32* zeros;         // >= 64 bytes of the kind's zero pattern (border of the first stripe)
    u32* work_counter;         // zeroed before the launch: next batch to hand out
    int32_t gex_mag;           // OFFS kernels: a = -gex; then gop holds encode_gap(gop - gex) and the profile s + a
    int32_t renorm_quads;      // OFFS: K/4 — the frame is lowered by a*K every K columns (uniform frame: every K steps; 0: never); a power of two
    u32 renorm_word;           // encode_gap(-a*K)
    u32 wrap_class;            // OFFS: encode_gap(-a*P), P = frame_classes(...) of the launched kernel (dp_step: row classes)
    u32 wrap_last;             // OFFS: encode_gap(-a*((R-1) % P + 1)); uniform frame: encode_gap(-a*((R-1) % P))
    int32_t* stat_count;       // optional.  Scan launches (streamed kernels): += subjects listed only because the slot before them
                               // scored at or above the zero-level jump (sw_set_dirty_counter).  Re-score launches: += subjects whose exact score is >= stat_limit, i.e. the
    int32_t stat_limit;        // reference's notion of an overflow (half2_kernels.cuh:1087-1109), for the printed statistic
    // Start handshake (side launches that must run BESIDE a grid that fills the GPU): every workgroup counts itself in
    // work_counter[1] when it becomes resident, and the one that completes start_quorum adds 1 to *start_signal (system
    // scope; signal memory a stream can wait on: hipStreamWaitValue32).  nullptr: no handshake.
    u32* start_signal;
    u32 start_quorum;
    // Overflow lists that are re-scored WHILE they are filled (sw_rescore_service).  claim: the list's entries are taken
    // with a compare-and-swap (-1: not written yet, >= 0: a subject to re-score, -2: taken), so that a service launch that
    // runs beside the producing launch and the ordinary re-score launch behind it never score an entry twice; the producer
    // publishes an entry with an agent-scope store (its plain stores would sit in its XCD's L2).  service: the list's length
    // (count_ptr) is polled per batch instead of read once, a batch is taken as soon as its first entry is there, and the
    // workgroup leaves when *done_flag has reached done_value (the producer has finished) and nothing is left for it.
    int32_t* claim;            // == positions, writable; nullptr: plain list
    int32_t service;
    const u32* done_flag;
    u32 done_value;
    // Tail hand-over (sw_set_dry_signal): the workgroup that finds the work counter dry — the first one that has nothing
    // left to take, while the others are still busy with their last batches — stores dry_value in *dry_signal (system
    // scope, signal memory).  A caller that ordered the NEXT query's launch behind that value on another stream gets a
    // grid that fills the slots this launch's workgroups leave one by one, instead of one that shares the CUs with it
    // from the start.  nullptr: none.
    u32* dry_signal;
    u32 dry_value;
    // Streamed subjects (sw_stream_kernel.hpp): batches a workgroup may claim at once (<= 1: sw_scan_kernel), the most columns
    // a round of several slots may have (the border scratch of multi-stripe queries is sized for it) and the most its
    // a * columns + jumps may add up to (the frame is not lowered inside such a round); the level of column -LANES (fp16
    // starts at the bottom of its exact range); what a lane's zero levels rise by at a slot border, and from which score of
    // the slot before on a slot is flagged (its lanes may have kept values above the raised levels)
    int32_t stream_slots;
    int32_t stream_cols;
    int32_t stream_room;
    int32_t level_base;
    int32_t jump;
    u32 jump_word;
    int32_t jump_limit;
    // Uniform frame (OFFS packed sw_scan_kernel, which needs a profile built with head_extra = 1): levels[u] = the zero level
    // a*u in the kind's packed encoding (Arith::zero_at), u <= K + P; the kernel reads its window with scalar loads
    int32_t uniform_frame;
    int32_t flag_period;       // the column frame's period K (offs_possible): the uniform frame flags at least what it would
    // Pair chains (packed multi-stripe sw_scan_kernel on 16-lane groups): a workgroup claims up to `chain` batches at once and
    // its groups walk their pairs of those batches back to back, as one virtual subject per stripe (sw_scan_kernel: "Pair
    // chains"; <= 1: one batch per claim); lcap and the scratch are sized for the chain (chain_region_words).  chain_all:
    // every claim takes `chain` batches (tests) — otherwise only while more than chain * grid batches remain
    int32_t chain;
    int32_t chain_all;
    u32 levels[kLevelWords];
};

constexpr int32_t kListEmpty = -1, kListTaken = -2;

typedef u32 u32x3 __attribute__((ext_vector_type(3)));

// chunk c of a lane's words for one letter (Chunks<NW>); c folds to a constant in the unrolled callers
template <int NW, int CHUNK_ROW_BYTES>
__device__ __forceinline__ void lds_read_chunk(u32 (&dst)[NW], const unsigned char* p, int c) {
    using C = Chunks<NW>;
    const int w = C::first(c);
    if (c < C::kN4) {
        const uint4 v = *reinterpret_cast<const uint4*>(p + c * CHUNK_ROW_BYTES);
        dst[w + 0] = v.x; dst[w + 1] = v.y; dst[w + 2] = v.z; dst[w + 3] = v.w;
    } else if (c < C::kCount) {
        const u32x3 v = *reinterpret_cast<const u32x3*>(p + c * CHUNK_ROW_BYTES);
        if constexpr (C::kSplit) {
            dst[w + 0] = v.x; dst[w + 1] = v.y; dst[w + 2] = v.z;
        } else {
            // NW = 1, 2, 5: one or two of the three words are used.  x passes through an empty asm that also takes the
            // unused words: a pure data dependency (no ordering against the hand-scheduled step) that keeps the compiler
            // from narrowing the load to a conflicting ds_read_b32 / b64 again
            u32 x = v.x;
            if constexpr (C::kRem == 1) asm("" : "+v"(x) : "v"(v.y), "v"(v.z));
            if constexpr (C::kRem == 2) asm("" : "+v"(x) : "v"(v.z));
            dst[w] = x;
            if constexpr (C::kRem == 2) dst[w + 1] = v.y;
        }
    }
}

template <int NW, int CHUNK_ROW_BYTES>
__device__ __forceinline__ void lds_read_words(u32 (&dst)[NW], const unsigned char* p) {
#pragma unroll
    for (int c = 0; c < Chunks<NW>::kCount; c++) lds_read_chunk<NW, CHUNK_ROW_BYTES>(dst, p, c);
}

// Row classes of the column-offset frame (dp_step<OFFS>): lane-local row r belongs to class r mod P and is kept raised
// by a further a * (r mod P).  P = 1 is the plain column frame.
// Packed single-stripe kernels up to this many rows per lane are bound to 168 VGPRs = three waves per SIMD (two waves
// fill 93.5 % of the issue slots at best, three 97 %: tools/ubench/dep_chain.hip); the multi-stripe kernels of the same
// height would spill (their border state), taller ones need the registers.
#ifndef SWK_WAVES3_MAX_R
#define SWK_WAVES3_MAX_R 36
#endif
#ifndef SWK_WAVES3_MAX_R_MULTI
// Packed MULTI-stripe kernels up to this many rows per lane are bound to 168 VGPRs as well (round 4).  With the stripe
// border in LDS rings (Border<LANES>) their loops run without a single scratch access at that bound (tools/loop_spills.py;
// what the code object reports as spills is set-up code), the 43 KB tile plus 8 KB of rings still fits three workgroups
// per CU, and the third wave is worth +6 % at the same stripe height (850 / 1000-residue queries: 10.8 / 11.0 -> 11.5 /
// 11.6 TCUPS) — enough for the planner to prefer 32-row stripes over 40..48-row ones for most long queries
// (sw_api.hip: plan_query; peak benchmark 11.53 -> 11.67 TCUPS).  0: none.
#define SWK_WAVES3_MAX_R_MULTI 32
#endif
#ifndef SWK_WAVES4_MAX_R
#define SWK_WAVES4_MAX_R 22   // ... and up to this many to 128 VGPRs = four waves per SIMD (+1 % at R = 17..22, -0.4 % at 24)
#endif
#ifndef SWK_CLASSES_PACKED
#define SWK_CLASSES_PACKED 8
#endif
#ifndef SWK_CLASSES_PACKED_SMALL
#define SWK_CLASSES_PACKED_SMALL 4
#endif
#ifndef SWK_CLASSES_SCALAR
#define SWK_CLASSES_SCALAR 4
#endif
constexpr int frame_classes(bool packed, int R, int lanes, bool multi, bool uniform = false) {
    (void)lanes;
    // packed kinds: 8 classes for the tall kernels (two waves per SIMD anyway: 0.125 instead of 0.25 wrap subtractions per
    // cell pair for 8 more registers, +0.8 % on the peak benchmark) and for the uniform-frame multi-stripe kernels from R = 25
    // on (their zero levels live in scalar registers: the registers of the column frame's level window pay for the four more
    // classes at three waves per SIMD — 779 instead of 791 VALU per quad at R = 32, no scratch access in the loop); the
    // single-stripe kernels up to R = SWK_WAVES3_MAX_R and everything below R = 25 four, which keeps those at three (or more)
    // waves per SIMD.  32-bit kinds: four (register-bound by their occupancy).
    const int want = packed ? ((R > SWK_WAVES3_MAX_R || (multi && R >= 25 && (uniform || R > SWK_WAVES3_MAX_R_MULTI))) ? SWK_CLASSES_PACKED : SWK_CLASSES_PACKED_SMALL)
                            : SWK_CLASSES_SCALAR;
    int P = want;
    while (P > 1 && 2 * P > R) P--;  // at least two rows per class, so that the running maximum still folds two rows per max3
    return P;
}

// Wide kernels: how many rows the diagonal terms run ahead of the chain in dp_step (8 and 16 measured within 0.1 %)
constexpr int kLookahead = 12;

// the words of two letters, chunk by chunk (A's chunk k, B's chunk k, ...): LDS answers in order, so the first rows'
// score words arrive after two reads instead of after all of A's
template <int NW, int CHUNK_ROW_BYTES>
__device__ __forceinline__ void lds_read_chunk2(u32 (&da)[NW], u32 (&db)[NW], const unsigned char* pa, const unsigned char* pb, int c) {
    lds_read_chunk<NW, CHUNK_ROW_BYTES>(da, pa, c);
    lds_read_chunk<NW, CHUNK_ROW_BYTES>(db, pb, c);
    __builtin_amdgcn_sched_barrier(0);  // keep this issue order (the scheduler would sort the reads by register)
}

template <int NW, int CHUNK_ROW_BYTES>
__device__ __forceinline__ void lds_read_words2(u32 (&da)[NW], u32 (&db)[NW], const unsigned char* pa, const unsigned char* pb) {
#pragma unroll
    for (int c = 0; c < Chunks<NW>::kCount; c++) lds_read_chunk2<NW, CHUNK_ROW_BYTES>(da, db, pa, pb, c);
}

// the same for one letter (32-bit kinds)
template <int NW, int CHUNK_ROW_BYTES>
__device__ __forceinline__ void lds_read_chunk1(u32 (&da)[NW], const unsigned char* pa, int c) {
    lds_read_chunk<NW, CHUNK_ROW_BYTES>(da, pa, c);
    __builtin_amdgcn_sched_barrier(0);
}

// Per-group DP state that lives across the steps of one stripe.
template <int KIND, int R, int P = 1>
struct StripeState {
    u32 H[R];      // H(row, column-1)
    u32 E[R];      // horizontal gap state entering the current column (clamped)
    u32 upH_prev;  // H(row0-1, column-1): diagonal input of the lane's first row
    u32 Hlast;     // H of the lane's bottom row after the last step
    u32 Fout;      // vertical gap state leaving the lane's bottom row after the last step
    u32 yA, yB;    // LDS byte address (+16 bias) of the lane's chunk for the current letter(s); packed kinds with
                   // 16-lane groups keep both in yA (B's address in the upper half)
    // OFFS: windows over the four steps of a quad.  With j0 the column the lane works on in the quad's first step,
    //   Zc[i]   = zero level of column j0 raised by a*i: step q uses Zc[q + k] for class k (or class + 1) — the zero levels
    //             of consecutive columns and classes are the same numbers, so nothing is added per step;
    //   maxv[d] = running maximum of all cells whose frame is a*(c_j0 + d): step q folds class c into maxv[q + c].
    // Both move up by 4a once per quad (2P + 7 additions instead of 8P per quad).  The plain form uses maxv[0] only.
    u32 maxv[P + 3];
    u32 Zc[P + 4];
};

// One anti-diagonal step of one lane: R cells (or R cell pairs).
//   BYTE    which byte of the letter words feeds lane 0 in this step
//   MULTI   stripe borders in play: lane 0 takes (inH, inF) — the previous stripe's bottom row at this
//           column — instead of the zero boundary; the caller stores lane 15's (Hlast, Fout) afterwards
//
// OFFS — the column-offset form of the recurrence.  With a = -gex all values of column j are kept as
// X* = X + a*c_j (c_j = j + LANES).  Then E*(i,j+1) = max3(E*(i,j), H* + (gop + a), Z_{j+1}) needs no addition of
// its own (E decays by a per column, the frame rises by a per column), F*(i+1,j) = max3(F*, H* + (gop + a), Z_{j+1}) - a,
// the diagonal term is H*(i-1,j-1) + (s + a) with the +a folded into the profile, and Z_j = a*c_j is the zero level
// of the column: 7.5 instead of 8.5 instructions per cell pair (6.5 instead of 7.5 per cell).  Price: one register
// (Z) and two instructions per step (Z += a; running maximum += a), and magnitudes
// that grow with the column index: the launcher picks OFFS only while a * columns stays well inside the exact range
// of the kind, and a subject whose bound maxscore + a * columns reaches the limit is flagged like an overflow.
// `first` (MULTI): the stripe has no predecessor, lane 0's boundary is the zero level instead of the border row.
// ZFILL = false (sw_stream_kernel.hpp): the head lane's vertical gap state is the column's zero level (class 0) instead of the
// bound_ctrl zero fill — levels that start below zero, and separator columns, which rebuild a lane's state from it.
// UNI (sw_scan_kernel, packed kinds): the uniform frame — the zero levels depend on the step alone and come from the caller's
// wave-uniform window zw (scalar registers) instead of st.Zc (sw_scan_kernel explains the frame).
// ADDR (packed kinds, 16-lane groups): lettersA is the lane's word of the address stream for this step (stream_region_words)
// and laneStep its slot byte 16 * slot; the two LDS addresses are one byte permute each, nothing travels along the group.
template <int KIND, int R, int LANES, int BYTE, bool MULTI, bool OFFS = false, int P = 1, bool ZFILL = true, bool UNI = false, bool ADDR = false>
__device__ __forceinline__ void dp_step(StripeState<KIND, R, P>& st, const unsigned char* tile,
                                        u32 lettersA, u32 lettersB, u32 gop, u32 gex, u32 inH, u32 inF,
                                        u32 apos = 0, bool first = false, u32 wrapP = 0, u32 wrapLast = 0, bool head = false,
                                        u32 laneStep = 0, const u32* zw = nullptr) {
    using A = Arith<KIND>;
    using G = Geometry<KIND, R, LANES>;
    // what a lane adds to the LDS address it receives: one 16-byte slot.  8-lane groups: the second group of a DPP row
    // works in slots 8..15 of the chunk row (the profile builder fills them with a copy), so its head lane adds 128 bytes
    // more — a per-lane constant (laneStep) in place of the literal, no instruction more.  With both groups in slots
    // 0..7 they met in the same banks with different letter rows: every second LDS cycle of the 8-lane kernels was a
    // conflict on ragged subjects.
    const u32 step2 = LANES < 16 ? laneStep : 0x00100010u;
    const u32 step1 = LANES < 16 ? laneStep : 16u;
    constexpr u32 kSel = 0x0c0c000cu | ((u32)BYTE << 8);  // letter byte BYTE -> bits 15:8
    constexpr int kPostShift = G::kLetterShift - 8;        // row offset = byte << kLetterShift

    static_assert(!A::kPacked || OFFS, "packed kinds run the column-offset recurrence only");
    // subject letter(s): shift along the group, lane 0 takes the next letter of its subject
    u32 wa[G::NW];
    u32 wb[G::NW];
    static_assert(!ADDR || (A::kPacked && LANES == 16 && OFFS), "the address stream serves the packed kinds on 16-lane groups");
    if constexpr (ADDR) {
        // (pa / pb below)
    } else if constexpr (A::kPacked && LANES <= 16) {
        // both LDS addresses (< 64 KB) travel in one register: one permute, one DPP move and one add for the pair
        constexpr u32 kSel2 = ((u32)(4 + BYTE) << 24) | 0x000c000cu | ((u32)BYTE << 8);  // B's byte -> 31:24, A's -> 15:8
        const u32 inj = __builtin_amdgcn_perm(lettersB, lettersA, kSel2);
        st.yA = prev_lane<LANES, false>(inj, st.yA, head) + step2;
    } else {
        const u32 injA = __builtin_amdgcn_perm(0u, lettersA, kSel) << kPostShift;
        st.yA = prev_lane<LANES, false>(injA, st.yA, head) + step1;
        // (32-bit kinds, column-offset form: progressive reads like the wide kernels, issued below)
        if constexpr (A::kPacked || !OFFS) lds_read_words<G::NW, G::kChunkRowBytes>(wa, tile + st.yA);
        if constexpr (A::kPacked) {
            const u32 injB = __builtin_amdgcn_perm(0u, lettersB, kSel) << kPostShift;
            st.yB = prev_lane<LANES, false>(injB, st.yB, head) + step1;
            lds_read_words<G::NW, G::kChunkRowBytes>(wb, tile + st.yB);
        }
    }

    if constexpr (OFFS) {
        // Row classes: lane-local row r (class p = r mod P) is kept raised by a further a*p.  F then needs its "- a" only
        // where the class wraps (every P rows, and after the lane's last row: by a*(p+1), back to class 0), E and F of a
        // row share the zero level Zc[Q+p+1], and the running maximum is kept per class (rows r and r+P fold into one
        // max3; StripeState explains the windows Zc / maxv and the step index Q).  What a lane passes on (Hlast) stays
        // in the frame of its last row's class; the profile entry of a row carries s + a*(1 + class - class of the row
        // above) (sw_build_profile_kernel), which makes row 0 consistent.
        constexpr int kLastClass = (R - 1) % P;
        constexpr int Q = A::kWindow ? BYTE : 0;  // step within the quad == which letter byte feeds lane 0
        u32 upH, F;
        if constexpr (MULTI) {
            // the stripe above's bottom row at this column; in the first stripe the IN ring holds the column's zero level as
            // H (the local-alignment boundary row 0's diagonal expects: first_stripe_pair) and the kind's unraised zero
            // pattern as F, which lies below every zero level — "no vertical gap" as well as any other value down there
            (void)first;
            upH = prev_lane<LANES, false>(inH, st.Hlast, head);
            F = prev_lane<LANES, false>(inF, st.Fout, head);
        } else {
            const u32 bH = UNI ? zw[Q + kLastClass] : st.Zc[Q + kLastClass];  // the local-alignment boundary H = 0 as row 0's diagonal expects it
            upH = prev_lane<LANES, false>(bH, st.Hlast, head);
            // any F below the column's zero level is "no vertical gap": bound_ctrl zero fill (pattern 0 is below every
            // zero level of every kind, and the fp16 comparator of the int16 kind orders +0.0 below all its patterns)
            if constexpr (ZFILL) F = prev_lane<LANES, true>(0u, st.Fout, head);
            else F = prev_lane<LANES, false>(st.Zc[Q], st.Fout, head);
        }
        u32 diag = st.upH_prev;
        st.upH_prev = upH;
        // the running maxima live in moving frames (st.maxv): the rows' maxima fold straight into the accumulator of
        // their frame (converted back to true scores once per stripe)
        u32 m[P];
#pragma unroll
        for (int c = 0; c < P; c++) m[c] = A::kWindow ? st.maxv[Q + c] : A::add(st.maxv[c], apos);
        // The rows are software-pipelined by hand: the chain h -> h+G -> max3 -> next row's h is serial, and on
        // gfx950 a packed op that reads the result of the instruction right before it costs a wait state, so the
        // independent work (score lookup and diagonal term of the rows ahead, the E update, the maximum) is
        // written in between the links of the chain.
        auto score = [&](int r) -> u32 {
            if constexpr (G::kWide) return 0u;
            else if constexpr (A::kPacked) return __builtin_amdgcn_perm(wb[r >> 1], wa[r >> 1], (r & 1) ? 0x07060302u : 0x05040100u);
            else return wa[r];
        };
        // diagonal term of a row: d + score (the wide kernels pair and add in one instruction, see tq below)
        auto diag_term = [&](int, u32 d, u32 sc) -> u32 { return A::add(d, sc); };
        // Wide words: the diagonal terms run kAhead rows ahead of the chain and the scheduler may only reorder within
        // four rows (it would otherwise compute all of them first, in register order, and so wait for the LAST LDS
        // chunk at the top of the step): a row needs its score words only when the chain is kAhead rows away.
        constexpr int kAhead = G::kWide ? (kLookahead < R ? kLookahead : R) : 1;
        // ... and the LDS reads themselves are issued progressively: the chunks the first kAhead + 4 rows need at the top
        // of the step, chunk k + kChunks0 when the chain reaches row 4k — a few chunks are in flight instead of all
        // (2R registers), which is what lets R go up to 48
        using CH = Chunks<G::NW>;
        constexpr int kChunksAll = CH::kCount;
        // with full chunks: the chunks of the first kAhead + 4 rows at the top (a read is issued at least four rows before
        // its first word is used), as many more as it takes where 3-word chunks shift the rows
        constexpr int kChunks0 = G::kWide ? CH::lead_for(kAhead, 4) : 1;
        static_assert(!G::kWide || kChunks0 >= kChunksAll || CH::lead_ok(kChunks0, kAhead, 4), "a score word would be used before its read is issued");
        // ADDR: byte 1 from the stream word (A: its byte 1, B: its byte 3), byte 0 the lane's slot; the +16 bias of the tile
        // (load_tile) is an immediate of the reads
        const unsigned char* const pa = ADDR ? tile + 16 + __builtin_amdgcn_perm(lettersA, laneStep, 0x0c0c0500u) : tile + (st.yA & 0xffffu);
        const unsigned char* const pb = ADDR ? tile + 16 + __builtin_amdgcn_perm(lettersA, laneStep, 0x0c0c0700u) : tile + (st.yA >> 16);
        u32 tq[G::kWide ? R : 1];
        if constexpr (G::kWide) {
#pragma unroll
            for (int k = 0; k < kChunks0 && k < kChunksAll; k++) lds_read_chunk2<G::NW, G::kChunkRowBytes>(wa, wb, pa, pb, k);
#pragma unroll
            for (int r = 0; r < kAhead; r++) tq[r] = A::add_pair(wa[r], wb[r], r == 0 ? diag : st.H[r - 1]);
        }
        constexpr bool kProg1 = !A::kPacked;
        // the score of row r + 2 is picked up when the chain is at row r: rows 0..7 at the top of the step when the chunks
        // are full ones, the chunk after those when the chain reaches a chunk's first row
        constexpr int kChunks0S = kProg1 ? CH::lead_for(2, 6) : 1;
        if constexpr (kProg1) {
#pragma unroll
            for (int k = 0; k < kChunks0S && k < kChunksAll; k++) lds_read_chunk1<G::NW, G::kChunkRowBytes>(wa, tile + st.yA, k);
        }
        u32 s_next = score(0);
        u32 t_next = G::kWide ? 0u : diag_term(0, diag, s_next);
        s_next = R > 1 ? score(1) : 0u;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int c = r % P;
            const u32 zop = UNI ? zw[Q + c + 2] : st.Zc[Q + c + 1];
            if constexpr (G::kWide) {
                if (r % 4 == 0) __builtin_amdgcn_sched_barrier(0);
                if (CH::starts_chunk(r) && CH::chunk_of(r) + kChunks0 < kChunksAll)
                    lds_read_chunk2<G::NW, G::kChunkRowBytes>(wa, wb, pa, pb, CH::chunk_of(r) + kChunks0);
                t_next = tq[r];
            }
            if constexpr (kProg1) {
                if (r % 4 == 0) __builtin_amdgcn_sched_barrier(0);
                if (CH::starts_chunk(r) && CH::chunk_of(r) + kChunks0S < kChunksAll)
                    lds_read_chunk1<G::NW, G::kChunkRowBytes>(wa, tile + st.yA, CH::chunk_of(r) + kChunks0S);
            }
            const u32 t = t_next;
            const u32 h = A::cell_h(t, st.E[r], F);
            const u32 s1 = s_next;
            if (r + 2 < R) s_next = score(r + 2);
            const u32 hg = A::gap(h, gop);  // gop + a
            if constexpr (G::kWide) {
                if (r + kAhead < R) tq[r + kAhead] = A::add_pair(wa[r + kAhead], wb[r + kAhead], st.H[r + kAhead - 1]);
            } else {
                if (r + 1 < R) t_next = diag_term(r + 1, st.H[r], s1);  // the row's old H is the next row's diagonal
            }
            const u32 fm = A::max3(F, hg, zop);
            st.E[r] = A::max3(st.E[r], hg, zop);
            if (r == R - 1) F = (UNI && kLastClass == 0) ? fm : A::gap(fm, wrapLast);  // the lane's last row: to class 0 of the next lane
            else if (c == P - 1) F = A::gap(fm, wrapP);  // class P-1 -> class 0: lower by a*P
            else F = fm;                                  // next class: frame rises by a while F decays by a
            if ((r / P) & 1) m[c] = A::fold2(m[c], st.H[r - P], h);
            else if (r + P >= R) m[c] = A::max2(m[c], h);
            st.H[r] = h;
        }
#pragma unroll
        for (int c = 0; c < P; c++) st.maxv[Q + c] = m[c];
        if constexpr (!A::kWindow) {
#pragma unroll
            for (int k = (kLastClass == 0 ? 0 : 1); k <= P; k++) st.Zc[k] = A::add(st.Zc[k], apos);
        }
        st.Hlast = st.H[R - 1];
        st.Fout = F;
    } else {
        // The plain recurrence (32-bit kinds only).  Row above the lane's first row: from the neighbouring lane, or from the
        // stripe border
        u32 upH, F;
        if constexpr (MULTI) {
            upH = prev_lane<LANES, false>(inH, st.Hlast, head);  // lane 0 keeps `old` == the border value
            F = prev_lane<LANES, false>(inF, st.Fout, head);
        } else {
            upH = prev_lane<LANES, true>(0u, st.Hlast, head);  // bound_ctrl zero fill == the local-alignment boundary
            F = prev_lane<LANES, true>(0u, st.Fout, head);
        }
        u32 diag = st.upH_prev;
        st.upH_prev = upH;

        u32 maxv = st.maxv[0];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const u32 t = A::add(diag, wa[r]);
            diag = st.H[r];
            const u32 h = A::cell_h(t, st.E[r], F);
            const u32 hg = A::gap(h, gop);
            st.E[r] = A::gap_state(A::gap(st.E[r], gex), hg);
            F = A::gap_state(A::gap(F, gex), hg);
            st.H[r] = h;
            // running maximum: folded two rows at a time (a 3-input max where the ISA has one)
            if (r & 1) maxv = A::fold2(maxv, st.H[r - 1], h);
            else if (r == R - 1) maxv = A::max2(maxv, h);
        }
        st.maxv[0] = maxv;
        st.Hlast = st.H[R - 1];
        st.Fout = F;
    }
}

// Copy one profile tile (global, L2-resident) into LDS.  The tile starts 16 bytes into the LDS
// array because lane addresses carry a +16 bias (lane 0 injects `offset`, lanes >0 add 16 per hop).
template <int TILE_BYTES>
__device__ __forceinline__ void load_tile(unsigned char* lds, const unsigned char* gsrc) {
    static_assert(TILE_BYTES % 16 == 0, "tile must be 16-byte granular");
    const uint4* src = reinterpret_cast<const uint4*>(gsrc);
    uint4* dst = reinterpret_cast<uint4*>(lds + 16);
    for (int i = threadIdx.x; i < TILE_BYTES / 16; i += kThreads) dst[i] = src[i];
}

// maximum over the 8 lanes of a half row, left in lanes 0..3 (and 8..11): half-row mirror, then the two quad swaps
template <class MAX>
__device__ __forceinline__ u32 half_row_max(u32 v, MAX&& mx) {
    v = mx(v, dpp<0x141, false>(v, v));  // row_half_mirror: lane i <-> 7 - i
    v = mx(v, dpp<0xB1, false>(v, v));   // quad_perm [1,0,3,2]
    v = mx(v, dpp<0x4E, false>(v, v));   // quad_perm [2,3,0,1]
    return v;
}

// ... and over the 4 lanes of a quad, left in all of them
template <class MAX>
__device__ __forceinline__ u32 quad_max(u32 v, MAX&& mx) {
    v = mx(v, dpp<0xB1, false>(v, v));   // quad_perm [1,0,3,2]
    v = mx(v, dpp<0x4E, false>(v, v));   // quad_perm [2,3,0,1]
    return v;
}

// maximum of true scores over the 16 lanes of a DPP row, left in all of them
template <int KIND>
__device__ __forceinline__ u32 row_max_true(u32 v) {
    using A = Arith<KIND>;
    v = A::true_max(v, dpp<0x128, false>(v, v));  // row_ror:8
    v = A::true_max(v, dpp<0x124, false>(v, v));  // row_ror:4
    v = A::true_max(v, dpp<0x122, false>(v, v));  // row_ror:2
    v = A::true_max(v, dpp<0x121, false>(v, v));  // row_ror:1
    return v;
}

// group maximum of the plain form (32-bit kinds)
template <int KIND, int LANES>
__device__ __forceinline__ u32 group_max(u32 v) {
    using A = Arith<KIND>;
    if constexpr (LANES == 8) return half_row_max(v, [](u32 a, u32 b) { return A::max2(a, b); });
    if constexpr (LANES == 4) return quad_max(v, [](u32 a, u32 b) { return A::max2(a, b); });
    v = row_max_true<KIND>(v);   // (32-bit kinds: their true scores compare like their values)
    if constexpr (LANES == 64) {
        v = A::max2(v, (u32)__shfl_xor((int)v, 16));
        v = A::max2(v, (u32)__shfl_xor((int)v, 32));
    }
    return v;
}

// ------------------------------------------------------------------------------------------------
// The scan kernel.  Persistent workgroups stride over batches of groups (LANES = 16: 16 groups, 32 or 16
// subjects per batch; LANES = 64: 4 groups), longest subjects first.  MULTI == the query needs more than
// one stripe.
// ------------------------------------------------------------------------------------------------
// Stripe border of multi-stripe queries (the analogue of the reference's devTempHcol2 / devTempEcol2,
// half2_kernels.cuh:335-338).  The bottom row of a stripe — one (H, F) pair = 8 bytes per subject column — goes from the
// group's LAST lane to lane 0 of the same group one stripe later.  Round 4: through LDS rings and block transfers.
//   * the last lane stores its pair into the group's OUT ring in LDS every step (one ds_write_b64; the other lanes hit
//     the group's dummy slot — stores of several lanes to ONE address do not serialise), lane 0 takes the previous stripe's
//     pair from the group's IN ring (one ds_read_b64; the other lanes read the same address and ignore the value): no
//     global access, no staging registers and no register copies in the step.  Round 6: the groups' rings are 16 bytes off
//     the 256-byte bank period and the dummy slots are per group, not per lane — the two groups a 64-bit LDS access serves
//     in one pass no longer meet in the same banks (SQ_LDS_BANK_CONFLICT of the R = 32 kernel: 2.38e9 -> 0.16e9 cycles per
//     launch of 2.8e10 LDS cycles; what is left are the steps on which a group's walking store meets its neighbour's dummy
//     slot);
//   * every kBlockCols = 2 * LANES steps the group moves one BLOCK: each lane copies 16 bytes of the OUT ring to the
//     global scratch (a fully coalesced 16 * LANES-byte burst: whole lines, written once) and 16 bytes of the block after
//     next from the scratch into a register, which it drops into the IN ring one block later.
// (Rounds 1-3: every lane issued 2 x 16-byte loads and stores per four steps, only lane 0's / the last lane's addresses
// walked the real array, the rest hit junk slots and the zeros array: 16 staging registers, ~3 register copies per step,
// and write-backs of junk lines.)  The scratch is indexed by the PRODUCER's step ("position"): the last lane emits column
// c at position c + LANES - 1, so the consumer's block b starts 8 * (LANES - 1) bytes into producer block b.
template <int LANES>
struct Border {
    static constexpr int kBlockCols = 2 * LANES;                 // positions per block: 16 bytes per lane
    static constexpr int kQuadsPerBlock = LANES / 2;
    static constexpr int kBlockBytes = 8 * kBlockCols;
    static constexpr int kBlockWords = 2 * kBlockCols;
    // LDS per group: IN ring and OUT ring, one block each; per workgroup one dummy slot per group (what they hold is never read)
    static constexpr int kInBytes = kBlockBytes, kOutBytes = kBlockBytes, kDummyBytes = 8 * (kThreads / LANES) + 32;   // one 8-byte dummy slot per group
    // + 16: a ds_read_b64 / ds_write_b64 of a wave is served 32 lanes at a time, i.e. two 16-lane groups per pass, and the
    // groups walk their rings in step — with rings 2^k bytes apart both groups' pairs sat in the same two banks on every step
    // (rounds 4-5: SQ_LDS_BANK_CONFLICT = 6.7 % of the multi-stripe kernels' LDS cycles, 0 in the single-stripe ones)
    static constexpr int kGroupBytes = kInBytes + kOutBytes + 16;
    static constexpr int ring_bytes(int groups) { return groups * kGroupBytes + kDummyBytes; }
    static_assert(kGroupBytes % 16 == 0, "rings are read and written 16 bytes at a time");
    // blocks of the global array for subjects of up to `steps` steps: the partial last block, the tail block behind it,
    // and one more that the consumer's look-ahead reads
    static constexpr int blocks(int steps) { return (steps + kBlockCols - 1) / kBlockCols + 3; }
};
template <int LANES>
constexpr int border_region_words(int lcap) { return Border<LANES>::blocks(lcap) * Border<LANES>::kBlockWords; }  // per group

// Address stream of the packed multi-stripe sw_scan_kernel on 16-lane groups (dp_step<ADDR>).  What a lane needs of the
// subject letters are the LDS addresses of two profile rows, and those are the same in every stripe of a subject pair: the
// group writes them ONCE per pair, one word per subject column behind its border array — bits 15:8 hold A's letter *
// kLetterUnits, bits 31:24 B's, the other two bytes are zero (what lane 0 injected into the systolic address register at
// every step of every stripe before) — and lane l reads the word of column t - l at step t.  Column 0 is word LANES of
// the stream; the words of columns -LANES .. -1 and of the columns behind a subject's end hold the padding letter, so a
// lane that has not reached the subject yet, or has left it, needs no special case.  Columns up to 4 * nquads + LANES - 1
// <= lcap + LANES - 5 are written: blocks(lcap) * kBlockCols >= lcap + 3 * kBlockCols words hold them.
template <int LANES>
constexpr int stream_region_words(int lcap) { return LANES == 16 ? Border<LANES>::blocks(lcap) * Border<LANES>::kBlockCols : 0; }
// scratch words per group: the border array, then the address stream
template <int LANES>
constexpr int group_region_words(int lcap) { return border_region_words<LANES>(lcap) + stream_region_words<LANES>(lcap); }

// Pair chains (sw_scan_kernel).  A chain of c pairs is one virtual subject: every pair but the last takes its longest
// subject's columns rounded up to whole quads — at least kChainMinCols, so that the four reset quads of one border lie
// before the first of the next — and four separator columns.  The border array and the address stream hold the virtual
// subject (lcap = border capacity of chain_columns); behind the regions of all groups of the grid lie the per-pair maxima:
// kChainMaxWords words per group, word 16 * k + lane = the running maximum (true scores) of pair k's cells in that lane.
constexpr int kChainMax = 8;
constexpr int kChainMinCols = 12;
constexpr int kChainMaxWords = (kChainMax - 1) * kGroup;
constexpr int chain_pair_columns(int lmax) { return ((lmax + 3) & ~3) < kChainMinCols ? kChainMinCols : ((lmax + 3) & ~3); }
constexpr int64_t chain_columns(int max_len, int c) { return (int64_t)(c - 1) * (chain_pair_columns(max_len) + 4) + max_len; }

// Start handshake (ScanParams::start_signal): this workgroup holds its registers and LDS now — whoever the caller ordered
// behind the signal cannot take them
__device__ __forceinline__ void announce_start(const ScanParams& p) {
    if (p.start_signal && threadIdx.x == 0) {
        if (atomicAdd(p.work_counter + 1, 1u) + 1u == p.start_quorum)
            __hip_atomic_fetch_add(p.start_signal, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Minimum waves per SIMD the register allocator must leave room for (2nd __launch_bounds__ argument).
// Packed kinds: 1 (unconstrained) is best — forcing 3-4 waves spills the multi-stripe kernels (-3..4 %).
// 32-bit kinds: v_add_f32/v_add_u32 co-issue with v_max3_* mostly ACROSS waves (tools/ubench/mix_rate.hip:
// 99 lanes/clk/CU at 4 waves/SIMD, 80 at 2), so they want occupancy more than registers.
#ifndef SWK_I32_WAVES3_MAX_R
#define SWK_I32_WAVES3_MAX_R 32
#endif
#ifndef SWK_I32_WAVES3_MAX_R_MULTI
#define SWK_I32_WAVES3_MAX_R_MULTI 32
#endif
#ifndef SWK_F32_WAVES3_MAX_R
#define SWK_F32_WAVES3_MAX_R 48
#endif
#ifndef SWK_F32_WAVES3_MAX_R_MULTI
#define SWK_F32_WAVES3_MAX_R_MULTI 48
#endif
constexpr int min_waves_of(int KIND, int R, int LANES, bool MULTI) {
    const bool packed = KIND == F16X2 || KIND == I16X2;
    // packed kinds: 2 waves/SIMD (256 VGPRs) for the tall kernels; up to SWK_WAVES3_MAX_R rows a third wave is asked for
    // (168 VGPRs): two waves cover each other's wait states only ~92 % of the time, three reach the issue peak
    if (packed && LANES <= 16 && MULTI && R <= SWK_WAVES3_MAX_R_MULTI) return 3;
    if (packed) return (LANES <= 16 && !MULTI && R <= SWK_WAVES4_MAX_R) ? 4 : (LANES <= 16 && !MULTI && R <= SWK_WAVES3_MAX_R) ? 3 : 2;
    // int32 above 32 rows per lane: two waves per SIMD (the registers of the taller stripes; its add/max3 mix cannot
    // co-issue anyway).  Up to 32 rows the third wave is worth more than the spills it causes in the multi-stripe kernels
    // from R = 24 up (two-stripe queries of 850 / 1000 residues: 6.36 / 6.42 with three waves, 6.12 / 6.22 TCUPS with two)
    if (KIND == I32 && LANES <= 16 && R > (MULTI ? SWK_I32_WAVES3_MAX_R_MULTI : SWK_I32_WAVES3_MAX_R)) return 2;
    if (KIND == F32 && LANES <= 16 && R > (MULTI ? SWK_F32_WAVES3_MAX_R_MULTI : SWK_F32_WAVES3_MAX_R)) return 2;
    // 4 would spill the multi-stripe R = 14..16 kernels; the wave-wide shape's 43 KB tiles cap it at 3 anyway
    return (R <= 16 && !MULTI && LANES <= 16) ? 4 : 3;
}
template <int KIND, int R, int LANES, bool MULTI>
constexpr int min_waves() { return min_waves_of(KIND, R, LANES, MULTI); }
// the vector registers a wave of that kernel may take: its slot in a SIMD's 512-entry register file (allocated in eights)
constexpr int vgpr_slot_of(int KIND, int R, int LANES, bool MULTI) { return (512 / min_waves_of(KIND, R, LANES, MULTI)) & ~7; }

template <int KIND, int R, int LANES, bool MULTI, bool OFFS = false>
__global__ void __launch_bounds__(kThreads, (min_waves<KIND, R, LANES, MULTI>())) sw_scan_kernel(const ScanParams p) {
    using A = Arith<KIND>;
    using G = Geometry<KIND, R, LANES>;
    constexpr int kGroups = kThreads / LANES;
    using BD = Border<LANES>;
    constexpr int SHL1 = Shift<LANES>::kShl1;
    constexpr int kQuadsPerLetterBlock = LANES;  // a lane holds 4 letters: LANES quads per reload
    static_assert(!A::kPacked || OFFS, "packed kinds run the column-offset recurrence only (sw_launch.hpp: launch_scan_ro)");
    constexpr bool kUni = A::kPacked;   // the packed kinds' frame (below)
    constexpr bool kAddr = A::kPacked && MULTI && LANES == 16;   // LDS addresses from the pair's address stream (stream_region_words)
    constexpr bool kChain = kAddr;      // pair chains (below): the launches of these kernels are plain ranges (launch_scan_ro)
    constexpr int P = OFFS ? frame_classes(A::kPacked, R, LANES, MULTI, kUni) : 1;  // row classes of the column-offset frame
    __shared__ __attribute__((aligned(16))) unsigned char lds[16 + G::kTileBytes];
    __shared__ int chainEnd[kChain ? (kThreads / 64) * kChainMax : 1];   // per wave: the virtual column behind pair k's last quad
    __shared__ __attribute__((aligned(16))) unsigned char rings[MULTI ? BD::ring_bytes(kGroups) : 16];

    const int tid = threadIdx.x;
    const int lane = tid & (LANES - 1);  // position in the alignment group
    const int group = tid / LANES;
    const bool head = lane == 0;
    // 8-lane groups: the two groups of a DPP row use the two halves of the row's 16 profile slots (dp_step: laneStep)
    // (4-lane groups likewise: the four groups of a row in slots 0..3, 4..7, 8..11, 12..15)
    const int slot = LANES < 16 ? (tid & 15) : lane;
    const u32 laneStep = kAddr ? 16u * (u32)slot : (A::kPacked ? 0x00100010u : 16u) * ((LANES < 16 && head) ? u32(slot + 1) : 1u);
    announce_start(p);
    // A re-score launch is the tail of its scan: a handful of subjects, each one group's walk, started BEHIND the bulk grid
    // whose older waves win the SIMD's arbitration — measured 0.27 us per step of a wave-wide fp32 group against 0.14 for
    // the same kernel launched ahead of the bulk grid.  Raised priority gives the walk its issue slots.
    if (p.positions) __builtin_amdgcn_s_setprio(2);
    const bool service = p.service != 0;  // uniform
    const int n = (p.count_ptr && !service) ? *p.count_ptr : p.n;  // service: the list's capacity; its length is polled per batch
    constexpr int kSubjPerBatch = kGroups * A::kSubjects;
    const int nbatches = (n + kSubjPerBatch - 1) / kSubjPerBatch;
    if (!service && (int)blockIdx.x >= nbatches) return;  // workgroup-uniform (device-side count of the re-score path)
    // Pair chains: claim c < nchain takes the batches kC * c .. kC * c + kC - 1 (the last one what is left of them), every
    // later claim one batch — one atomic per claim either way.  Unless chain_all lifts the rule, a claim is a chain only
    // while more than kC * gridDim.x batches remain: the last rounds of a launch hand out single batches as before, so the
    // workgroups still finish within one pair's walk of each other
    const int kC = kChain ? min(max(p.chain, 1), kChainMax) : 1;
    const int nchain = (!kChain || kC == 1) ? 0 : p.chain_all ? (nbatches + kC - 1) / kC : max(0, (nbatches - kC * (int)gridDim.x + kC - 1) / kC);
    const int nclaims = kChain ? nchain + max(0, nbatches - nchain * kC) : nbatches;

    if constexpr (!MULTI) {
        load_tile<G::kTileBytes>(lds, p.profile);
        __syncthreads();
    }

    // Stripe border of this group (Border<LANES>): its rings in LDS and its block array in the global scratch
    unsigned char* const ringIn = rings + (MULTI ? group * BD::kGroupBytes : 0);
    unsigned char* const ringOut = ringIn + BD::kInBytes;
    u32* const gBorder = MULTI ? p.scratch + ((size_t)blockIdx.x * kGroups + group) * (size_t)group_region_words<LANES>(p.lcap) : nullptr;
    // Address stream of this group (stream_region_words), as the loop reads it: the stream of the wave's first group — a
    // wave-uniform base, which lives and walks in scalar registers — and this lane's byte offset from it at step 0: column
    // -lane of its own group's stream (the groups of a wave lie < 4 GB apart: a region is a few words per column)
    // (a global-memory pointer by type: rebuilt from integers it would be a generic one, whose loads count in lgkmcnt too)
    typedef const __attribute__((address_space(1))) unsigned char* StreamPtr;
    StreamPtr streamBase = nullptr;
    u32 streamOff = 0;
    if constexpr (kAddr) {
        constexpr int kGroupsPerWave = 64 / LANES;
        const int g0 = group & ~(kGroupsPerWave - 1);
        const uintptr_t b = reinterpret_cast<uintptr_t>(p.scratch + ((size_t)blockIdx.x * kGroups + g0) * (size_t)group_region_words<LANES>(p.lcap) +
                                                        border_region_words<LANES>(p.lcap));
        streamBase = (StreamPtr)(((uintptr_t)(u32)__builtin_amdgcn_readfirstlane((int)(b >> 32)) << 32) |
                                 (uintptr_t)(u32)__builtin_amdgcn_readfirstlane((int)(u32)b));
        streamOff = 4u * (u32)((group - g0) * group_region_words<LANES>(p.lcap) + LANES - lane);
    }

    // The frame of the column-offset recurrence (dp_step<OFFS>).
    //   * 32-bit kinds: the column frame — a cell of column j is raised by a*(j + LANES), a lane starts every stripe "at
    //     column -lane" (zero level a*(LANES - lane)) and keeps its own zero levels (st.Zc); no lowering (a 32-bit frame has
    //     room for any subject);
    //   * packed kinds: the UNIFORM frame — a cell of step t of stripe s is raised by a*(u + 1 + class), u = t_g mod K with
    //     t_g = t + LANES*s the global anti-diagonal.  A lane's column is t - lane, so the frame of a cell is a function of
    //     its column and its global lane index LANES*s + lane: from column j to j + 1 the frame rises by a (E needs no
    //     addition), the row classes work as in the column frame, a hand-off to the next lane (same column, one step
    //     later) raises it by a*(1 - lastClass) (F: wrap_last = a*lastClass; row 0's diagonal, two steps back: the profile
    //     carries a*(2 - lastClass), head_extra = 1), and a stripe border is one more such hand-off: t_g continues across it,
    //     the border rings need no correction.  The zero levels are the same in every lane of the wave: a window zw of
    //     P + 5 words in scalar registers, zw[k] = a*(u0 + k) with u0 the u of the quad's first step (ScanParams::levels),
    //     and at u = K - 1 every lane lowers all it holds by a*K in the same step, after the quad's last step.
    const u32 apos = OFFS ? A::pos_word(p.gex_mag) : 0u;
    const u32 apos4 = OFFS ? A::pos_word(4 * p.gex_mag) : 0u;
    const int rq = kUni ? p.renorm_quads : 0;
    const int kmask = 4 * rq - 1;   // kUni: u = t_g & kmask
    const u32 zstart = (OFFS && !kUni) ? A::zero_at(p.gex_mag, LANES - lane) : A::kZero;
    const u32 zbefore = (OFFS && !kUni) ? A::zero_at(p.gex_mag, LANES - lane - 1) : A::kZero;  // the column before

    __shared__ int next_batch, batch_avail;
    // an entry of a claimed list: wait (briefly: the producer stores it right after it has counted it) until it is written,
    // then take it; -1: somebody else has it
    auto claim_entry = [&](int i) -> int {
        for (int spin = 0; spin < (1 << 20); spin++) {
            const int v = __hip_atomic_load(p.claim + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v == kListTaken) return -1;
            if (v >= 0) return atomicCAS(p.claim + i, v, kListTaken) == v ? v : -1;
            __builtin_amdgcn_s_sleep(2);
        }
        return -1;
    };
    for (;;) {
        // dynamic batch distribution: one atomic per workgroup per batch
        __syncthreads();
        if (tid == 0) {
            int b = (int)atomicAdd(p.work_counter, 1u), avail = n;
            if (service) {
                // the batch is there as soon as its first entry is; the producer's end (done_flag) ends the wait — what the
                // service has not taken by then is the ordinary re-score launch's
                avail = 0;
                for (u32 spin = 0; b < nbatches; spin++) {
                    avail = __hip_atomic_load(p.count_ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (avail > b * kSubjPerBatch) break;
                    const u32 done = __hip_atomic_load(p.done_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    if ((int32_t)(done - p.done_value) >= 0 || spin > 600000u) { b = nbatches; break; }  // (the bound, ~2 s: never hang a GPU on a lost flag; what is left goes to the ordinary re-score launch)
                    __builtin_amdgcn_s_sleep(127);
                }
                avail = min(avail, n);
            }
            if (b == nclaims && p.dry_signal) __hip_atomic_store(p.dry_signal, p.dry_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            next_batch = b;
            batch_avail = avail;
        }
        __syncthreads();
        const int b = next_batch;
        if (b >= nclaims) break;
        const int navail = batch_avail;
        // the claim's batches in hand-out order: hb .. hb + cnt - 1 (kChain: a chain of cnt pairs per group; else the one batch)
        int hb = b, cnt = 1;
        if constexpr (kChain) {
            if (b < nchain) { hb = kC * b; cnt = min(kC, nbatches - hb); }
            else hb = nchain * kC + (b - nchain);
            hb = __builtin_amdgcn_readfirstlane(hb);
            cnt = __builtin_amdgcn_readfirstlane(cnt);
        }
        // a group's pair of subjects of one batch; lmax: the longest subject of the wave's groups (they run in lock-step)
        struct Pair {
            bool valid0 = false, valid1 = false;
            int pos0 = 0, pos1 = 0, len0 = 0, len1 = 0, lmax = 0;
            const int8_t* s0 = nullptr;
            const int8_t* s1 = nullptr;
        };
        auto load_pair = [&](int hbk) -> Pair {
            Pair r;
            const int batch = service ? hbk : nbatches - 1 - hbk;  // DB is length-sorted ascending: longest first; a service walks its list as it grows
            const int i0 = batch * kSubjPerBatch + group * A::kSubjects;
            const int i1 = i0 + 1;
            r.valid0 = i0 < navail;
            r.valid1 = A::kPacked && (i1 < navail);
            r.s0 = p.chars;
            r.s1 = p.chars;
            if (p.claim) {  // (32-bit kinds only: one subject per group; read by the group's lane 0, broadcast below)
                int v = -1;
                if (r.valid0 && lane == 0) v = claim_entry(i0);
                if constexpr (LANES == 64) v = __builtin_amdgcn_readfirstlane(v);
                else v = __shfl(v, (tid & 63) & ~(LANES - 1));
                r.valid0 = v >= 0;
                r.pos0 = r.valid0 ? v : 0;
                if (r.valid0) {
                    r.len0 = p.lengths[r.pos0];
                    r.s0 = p.chars + (p.offsets[r.pos0] - p.offsets[0]);
                }
                r.valid1 = false;
            } else {
                if (r.valid0) {
                    r.pos0 = p.positions ? p.positions[i0] : p.first_pos + i0;
                    r.len0 = p.lengths[r.pos0];
                    r.s0 = p.chars + (p.offsets[r.pos0] - p.offsets[0]);
                }
                if (r.valid1) {
                    r.pos1 = p.positions ? p.positions[i1] : p.first_pos + i1;
                    r.len1 = p.lengths[r.pos1];
                    r.s1 = p.chars + (p.offsets[r.pos1] - p.offsets[0]);
                }
            }
            // a caller that under-reports the longest subject (include/cudasw4_amd.h: max_subject_len): the subject ends at the
            // bound — its letters (whole words: len_bound is a multiple of 4), its walk and its place in a chain are those
            // of its first len_bound residues
            if constexpr (MULTI) {
                r.len0 = min(r.len0, p.len_bound);
                r.len1 = min(r.len1, p.len_bound);
            }
            int lmax = r.len0 > r.len1 ? r.len0 : r.len1;
            if constexpr (LANES <= 16) {  // the 4 (8) groups of a wave run in lock-step
                if constexpr (LANES <= 4) lmax = max(lmax, __shfl_xor(lmax, 4));
                if constexpr (LANES <= 8) lmax = max(lmax, __shfl_xor(lmax, 8));
                lmax = max(lmax, __shfl_xor(lmax, 16));
                lmax = max(lmax, __shfl_xor(lmax, 32));
            }
            r.lmax = lmax;
            return r;
        };
        // (kChain: the pairs are looked up where they are needed — when the stream is written and when the scores are — so
        // that nothing of them lives in registers across the stripes)
        Pair pr;
        if constexpr (!kChain) pr = load_pair(hb);
        const bool valid0 = pr.valid0, valid1 = pr.valid1;
        const int pos0 = pr.pos0, pos1 = pr.pos1, len0 = pr.len0, len1 = pr.len1;
        const int8_t* const s0 = pr.s0;
        const int8_t* const s1 = pr.s1;
        // the last lane finishes column lmax-1 at step lmax+LANES-2
        int nquads = (pr.lmax + LANES - 1 + 3) >> 2;
        // the border arrays hold lcap columns (sized from the caller's max_subject_len): never walk past them (load_pair has
        // cut a longer subject at the bound, so this clamp does not engage: it stays as the last line of defence)
        if constexpr (MULTI) nquads = min(nquads, (p.lcap - 4) >> 2);
        // the same in every lane of the wave (lmax was reduced over its groups): saying so turns the quad loop, its
        // letter-reload test and the frame-lowering segments into scalar control flow (the counter otherwise lives in a
        // VGPR, with a compare, an exec update and a masked branch per quad).  Single-stripe kernels: +0.5 %.  The
        // multi-stripe kernels do the same: rounds 1-3 kept their counters in vector registers (the scalar form measured 1 %
        // slower then); with the block loop of the LDS border rings it is the faster one (11.39 -> 11.44 TCUPS) and frees
        // registers
        nquads = __builtin_amdgcn_readfirstlane(nquads);
        const int len0pad = (len0 + 3) & ~3, len1pad = (len1 + 3) & ~3;
        // letters j .. j + 3 of a subject (j a multiple of 4: one aligned word; the padding letter behind its end), premultiplied
        // by kLetterUnits so that a byte << kLetterShift is the byte offset of the letter's profile row
        auto letters4 = [&](const int8_t* s, int lenpad, int j) -> u32 {
            u32 w = 0x14141414u;
            if (j < lenpad) w = *reinterpret_cast<const u32*>(s + j);
            return w * (u32)G::kLetterUnits;
        };
        if constexpr (kAddr) {
            // The address stream (stream_region_words), once for all stripes: lane l writes the four words of a pair's columns
            // 4c .. 4c + 3 for c = l, l + LANES, ..., and the padding word of column l - LANES.  Each subject pads from its own
            // end; a group without a subject B has len1 = 0.  A chain's pairs lie one behind the other, pair k from virtual
            // column col0 on: its chain_pair_columns(lmax) columns and the separator quad (padding: behind both subjects'
            // ends); the last pair as a single pair always was, up to column 4 * nquads + LANES - 1 of the virtual subject.
            u32* const sw = gBorder + border_region_words<LANES>(p.lcap) + LANES;   // the word of column 0
            const int wcap = 4 * ((p.lcap - 4) >> 2) + LANES;                        // columns the region holds for the longest walk
            sw[lane - LANES] = (u32)(kPadLetter * G::kLetterUnits) * 0x01000100u;
            auto put4 = [&](const Pair& q, int col0, int c) {
                if (col0 + 4 * c + 4 > wcap) return;   // (a caller that under-reports the longest subject)
                const u32 a = letters4(q.s0, (q.len0 + 3) & ~3, 4 * c), b = letters4(q.s1, (q.len1 + 3) & ~3, 4 * c);
                // B's byte k -> bits 31:24, A's -> bits 15:8
                *reinterpret_cast<uint4*>(sw + col0 + 4 * c) = make_uint4(__builtin_amdgcn_perm(b, a, 0x040c000cu), __builtin_amdgcn_perm(b, a, 0x050c010cu),
                                                                          __builtin_amdgcn_perm(b, a, 0x060c020cu), __builtin_amdgcn_perm(b, a, 0x070c030cu));
            };
            int col0 = 0;
            for (int k = 0; k + 1 < cnt; k++) {
                const Pair q = load_pair(hb + k);
                const int T = chain_pair_columns(__builtin_amdgcn_readfirstlane(q.lmax));
                for (int c = lane; c < T / 4 + 1; c += LANES) put4(q, col0, c);
                if ((tid & 63) == 0) chainEnd[(tid >> 6) * kChainMax + k] = col0 + T;
                col0 += T + 4;
            }
            const Pair q = load_pair(hb + cnt - 1);
            nquads = (col0 + __builtin_amdgcn_readfirstlane(q.lmax) + LANES - 1 + 3) >> 2;
            nquads = __builtin_amdgcn_readfirstlane(min(nquads, (p.lcap - 4) >> 2));
            for (int c = lane; c < nquads - col0 / 4 + LANES / 4; c += LANES) put4(q, col0, c);
            // the group's own lanes read it, from the first stripe's acquire fence on (the border arrays travel the same way)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        }

        u32 maxv = 0u;  // true scores (the plain form, 32-bit kinds only, has no bias either)
        for (int stripe = 0; stripe < p.nstripes; stripe++) {
            const bool first = stripe == 0;
            if constexpr (MULTI) {
                __syncthreads();
                load_tile<G::kTileBytes>(lds, p.profile + (size_t)stripe * G::kTileBytes);
                __syncthreads();
            }
            StripeState<KIND, R, P> st;
            // kUni: the level window of the quad to come (scalar loads from the kernel arguments).  Used as operands right after
            // the loads, so that the wait for them falls here and not among the LDS reads of the next step.
            u32 zw[P + 5];
            const int tg0 = kUni ? __builtin_amdgcn_readfirstlane(LANES * stripe) : 0;   // t_g of the stripe's first step
            auto load_levels = [&](int q) {
                const int u0 = __builtin_amdgcn_readfirstlane((tg0 + 4 * q) & kmask);
#pragma unroll
                for (int k = 0; k < P + 5; k++) zw[k] = p.levels[u0 + k];
#pragma unroll
                for (int k = 0; k < P + 5; k++) asm volatile("" : "+s"(zw[k]));
            };
            if constexpr (kUni) {
                load_levels(0);
                // the state before the first step (t_g0 - 1): H at its zero level, E at the level of the first step
#pragma unroll
                for (int r = 0; r < R; r++) { st.H[r] = zw[r % P]; st.E[r] = zw[r % P + 1]; }
                // upH_prev: the boundary H(row above, column before) of the first step's row 0 — the previous lane's last row
                // two steps back, one level below zw[lastClass] (fp16: may be -a; int16: >= 1024 - a)
                st.upH_prev = A::gap(zw[(R - 1) % P], p.gex); st.Hlast = zw[(R - 1) % P]; st.Fout = zw[0];
                // accumulator d holds the cells of frame zw[d + 1] (step q, class c: d = q + c); true score -> that frame
                // (a chain starts with its first pair: maxv is its last pair's)
                const u32 seed = (kChain && cnt > 1) ? 0u : maxv;
#pragma unroll
                for (int d = 0; d < P + 3; d++) st.maxv[d] = A::add(seed, zw[d + 1]);
            } else {
                // zero levels of the column before the lane's first one, per class (zc[k] = zbefore + a*k)
                u32 zc[P + 5];
                zc[0] = zbefore; zc[1] = zstart;
#pragma unroll
                for (int k = 2; k < P + 5; k++) zc[k] = A::add(zc[k - 1], apos);
#pragma unroll
                for (int r = 0; r < R; r++) { st.H[r] = zc[r % P]; st.E[r] = zc[r % P + 1]; }
                st.upH_prev = zc[(R - 1) % P]; st.Hlast = zc[(R - 1) % P]; st.Fout = zbefore;
#pragma unroll
                for (int k = 0; k < P + 4; k++) st.Zc[k] = zc[k + 1];
                // OFFS: true score -> frame of the column before the first
#pragma unroll
                for (int d = 0; d < P + 3; d++) st.maxv[d] = OFFS ? A::add(maxv, zc[A::kWindow ? d + 1 : d]) : maxv;
            }
            st.yA = ((u32)(kPadLetter * G::kLetterUnits) << G::kLetterShift) + 16u * (u32)(slot + 1);
            st.yB = st.yA;
            if constexpr (A::kPacked && LANES <= 16) st.yA |= st.yA << 16;  // (address for subject B, address for subject A)

            // subject letters: lane l holds letters 4*LANES*blk + 4l .. +3 of each subject, premultiplied
            // by kLetterUnits so that a byte << kLetterShift is the byte offset of the letter's profile row
            auto fetch = [&](const int8_t* s, int lenpad, int blk) -> u32 {
                if constexpr (kAddr) return 0u;   // (the address stream has them)
                else return letters4(s, lenpad, blk * (4 * LANES) + lane * 4);
            };
            u32 nextA = fetch(s0, len0pad, 0);
            u32 nextB = A::kPacked ? fetch(s1, len1pad, 0) : 0u;
            u32 lettersA = 0, lettersB = 0;
            // kAddr: the stream as this stripe walks it — the scalar base moves on by four words per quad, the steps of a quad
            // are immediate offsets — and the word of the step to come, requested one step ahead like the border pair (nxt)
            StreamPtr streamAt = streamBase;
            auto stream_word = [&](int k) -> u32 { return ((const __attribute__((address_space(1))) u32*)(streamAt + (size_t)streamOff))[k]; };
            u32 nxtW = 0;

            // Stripe border (MULTI only; Border<LANES>).  Lane 0 walks the IN ring, the last lane the OUT ring; the other
            // lanes read the ring's first pair over and over and write into their dummy slots.
            const bool last = stripe + 1 == p.nstripes;
            const unsigned char* inPtr = ringIn;
            unsigned char* outPtr = (lane == LANES - 1) ? ringOut : rings + kGroups * BD::kGroupBytes + 8 * group;
            const u32 walkIn = 32u;   // bytes per quad; every lane reads along with lane 0 (one address per group: a broadcast)
            const u32 walkOut = (lane == LANES - 1) ? 32u : 0u;
            uint4 pend = make_uint4(A::kZero, A::kZero, A::kZero, A::kZero);   // this lane's 16 bytes of the block after the current one
            uint2 nxt = make_uint2(A::kZero, A::kZero);                          // the pair of the step to come
            // consumer block b = positions b * kBlockCols + (LANES - 1) ...: 8 * (LANES - 1) bytes into producer block b
            const u32* const gIn = MULTI ? gBorder + 2 * (LANES - 1) + 4 * lane : nullptr;
            // What lane 0 takes in the FIRST stripe, where no stripe lies above: columns j, j + 1 -> (H, F, H, F) with H the
            // local-alignment boundary in the frame row 0's diagonal term expects — kUni: the zero level of the step before
            // (t_g = j - 1) in the class of a lane's last row, a * ((j mod K) + lastClass); column frame: a * (j + LANES +
            // lastClass); plain form: the kind's zero — and F "no vertical gap"
            auto first_stripe_pairs = [&](int j) -> uint4 {
                if constexpr (kUni) {
                    constexpr int kLastClass = (R - 1) % P;
                    return make_uint4(A::zero_at(p.gex_mag, (j & kmask) + kLastClass), A::kZero, A::zero_at(p.gex_mag, ((j + 1) & kmask) + kLastClass), A::kZero);
                } else if constexpr (OFFS) {
                    constexpr int kLastClass = (R - 1) % P;
                    const int K = 4 * rq;   // frame period (0: the frame is never lowered)
                    const int j0 = K > 0 ? (j & (K - 1)) : j, j1 = K > 0 ? ((j + 1) & (K - 1)) : j + 1;
                    return make_uint4(A::zero_at(p.gex_mag, j0 + LANES + kLastClass), A::kZero, A::zero_at(p.gex_mag, j1 + LANES + kLastClass), A::kZero);
                } else {
                    return make_uint4(A::kZero, A::kZero, A::kZero, A::kZero);
                }
            };
            if constexpr (MULTI) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                if (!first) {
                    const uint4 b0 = *reinterpret_cast<const uint4*>(gIn);
                    pend = *reinterpret_cast<const uint4*>(gIn + BD::kBlockWords);
                    *reinterpret_cast<uint4*>(ringIn + 16 * lane) = b0;
                } else {
                    *reinterpret_cast<uint4*>(ringIn + 16 * lane) = first_stripe_pairs(2 * lane);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                nxt = *reinterpret_cast<const uint2*>(inPtr);
                if constexpr (kAddr) nxtW = stream_word(0);
            }
            // end of block `blk` (all of its steps are done): the OUT ring's first block goes to the scratch, the IN ring
            // takes the next block, the load of the one after that is issued
            auto block_end = [&](int blk) {
                // every address is rebuilt here from the thread index (kept opaque, so that the compiler does not hoist a
                // dozen loop-invariant address registers into a loop that runs at the register limit)
                int t = tid;
                asm volatile("" : "+v"(t));
                const int ln = t & (LANES - 1), grp = t / LANES;
                unsigned char* const rIn = rings + grp * BD::kGroupBytes + 16 * ln;
                u32* const gb = p.scratch + ((size_t)blockIdx.x * kGroups + grp) * (size_t)group_region_words<LANES>(p.lcap) + 4 * ln;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                if (!last) {
                    const uint4 v = *reinterpret_cast<const uint4*>(rIn + BD::kInBytes);
                    *reinterpret_cast<uint4*>(gb + (size_t)blk * BD::kBlockWords) = v;
                }
                outPtr -= walkOut * BD::kQuadsPerBlock;
                inPtr -= walkIn * BD::kQuadsPerBlock;
                if (first) {
                    *reinterpret_cast<uint4*>(rIn) = first_stripe_pairs((blk + 1) * BD::kBlockCols + 2 * ln);
                } else {
                    *reinterpret_cast<uint4*>(rIn) = pend;
                    pend = *reinterpret_cast<const uint4*>(gb + 2 * (LANES - 1) + (size_t)(blk + 2) * BD::kBlockWords);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                nxt = *reinterpret_cast<const uint2*>(inPtr);   // what the last step prefetched was the old block's
            };

            // kUni: every lane lowers its frame by a*K after the last step of a frame period (u = K - 1) — H, E, the values in
            // flight to the next lane and the next step (Hlast, Fout, upH_prev) and the running maxima — BEFORE the last lane
            // stores its pair into the OUT ring, so that the next stripe's lane 0, one step later, reads it in its own frame
            auto lower_frame = [&]() {
                if constexpr (kUni) {
                    const u32 w = p.renorm_word;
#pragma unroll
                    for (int r = 0; r < R; r++) { st.H[r] = A::lower(st.H[r], w); st.E[r] = A::lower(st.E[r], w); }
                    st.upH_prev = A::lower(st.upH_prev, w);
                    // int16: lane 0's diagonal may be a border ring's "no value" (the bias, level 0), which a*K > 1024 takes
                    // below 0 and the next diagonal addition would wrap into the NaN patterns.  Every real value it can
                    // hold lies at or above level - a (the boundary at lastClass 0): the floor keeps "no value" below them.
                    if constexpr (KIND == I16X2) st.upH_prev = A::true_max(st.upH_prev, A::gap(A::kZero, p.gex));
                    st.Hlast = A::lower(st.Hlast, w);
                    st.Fout = A::lower(st.Fout, w);
#pragma unroll
                    for (int d = 0; d < P + 3; d++) st.maxv[d] = A::lower(st.maxv[d], w);
                }
            };
            auto quad = [&](int q) {
                if (!kAddr && (q & (kQuadsPerLetterBlock - 1)) == 0) {
                    lettersA = nextA; lettersB = nextB;
                    nextA = fetch(s0, len0pad, q / kQuadsPerLetterBlock + 1);
                    if constexpr (A::kPacked) nextB = fetch(s1, len1pad, q / kQuadsPerLetterBlock + 1);
                }
                const bool lower = kUni && ((tg0 + 4 * q + 4) & kmask) == 0;   // wave-uniform
                // one step: lane 0's pair of the stripe above from the IN ring, the last lane's own pair into the OUT ring.
                // The pair is requested ONE STEP AHEAD (nxt): the chain of a step starts with it (row 0's diagonal and F),
                // and an LDS read issued at the top of the step would be waited for right there.
                auto border_step = [&](auto byte_tag) {
                    constexpr int BYTE = decltype(byte_tag)::value;
                    const uint2 in = nxt;
                    if constexpr (MULTI) {
                        if constexpr (BYTE == 3) {
                            inPtr += walkIn;
                            nxt = *reinterpret_cast<const uint2*>(inPtr);   // first pair of the next quad (re-read after a block transfer)
                        } else {
                            nxt = *reinterpret_cast<const uint2*>(inPtr + 8 * (BYTE + 1));
                        }
                    }
                    if constexpr (kAddr) {
                        lettersA = nxtW;
                        if constexpr (BYTE == 3) {
                            streamAt += 16;
                            nxtW = stream_word(0);
                        } else {
                            nxtW = stream_word(BYTE + 1);
                        }
                    }
                    dp_step<KIND, R, LANES, BYTE, MULTI, OFFS, P, true, kUni, kAddr>(st, lds, lettersA, lettersB, p.gop, p.gex, in.x, in.y, apos, first,
                                                                                 p.wrap_class, p.wrap_last, head, laneStep, zw);
                    if constexpr (kUni && BYTE == 3) {
                        if (lower) lower_frame();
                    }
                    if constexpr (MULTI) *reinterpret_cast<uint2*>(outPtr + 8 * BYTE) = make_uint2(st.Hlast, st.Fout);
                };
                border_step(std::integral_constant<int, 0>{});
                border_step(std::integral_constant<int, 1>{});
                border_step(std::integral_constant<int, 2>{});
                border_step(std::integral_constant<int, 3>{});
                if constexpr (MULTI) outPtr += walkOut;
                if constexpr (!kAddr) {
                    lettersA = dpp<SHL1, true>(0u, lettersA);
                    if constexpr (A::kPacked) lettersB = dpp<SHL1, true>(0u, lettersB);
                }
                if constexpr (OFFS && A::kWindow) {  // the windows move on by four columns (kUni: steps; its levels are scalar)
                    if constexpr (!kUni) {
#pragma unroll
                        for (int k = 0; k < P + 4; k++) st.Zc[k] = A::add(st.Zc[k], apos4);
                    }
#pragma unroll
                    for (int d = 0; d < P + 3; d++) st.maxv[d] = A::add(st.maxv[d], apos4);
                }
                if constexpr (kUni) load_levels(q + 1);
            };
            // Pair chains: the hand-over from pair k to pair k + 1 of the virtual subject.  Pair k ends at virtual column E
            // (chainEnd), four separator columns of the padding letter follow, pair k + 1 starts at column E + 4: lane l works on
            // its last column of pair k at step E - 1 + l and on its first of pair k + 1 at step E + 4 + l, so the lanes 4j ..
            // 4j + 3 are between the two at the top of quad E / 4 + j + 1 — where reset_lanes(k, j) turns them into the lanes
            // of a fresh subject, under one exec mask and outside the four-step body:
            //   * their maxima window becomes true scores (as at a stripe's end), which join the pair's running maximum of
            //     the stripes above in the scratch (kChainMaxWords), and is seeded again at the levels of the quad to come;
            //   * H, E, upH_prev, Hlast and Fout become what the stripe prologue sets: the state before this step of a lane
            //     that has seen padding only.
            // Everything else runs on across the border: the uniform frame and its lowering, the address stream, the border
            // rings and blocks (positions of the virtual subject).  What a lane computes on separator columns before its reset
            // continues pair k behind its end, like the padding behind a single pair (it raises no maximum); behind the reset
            // it keeps the fresh state.  Lane 4j takes the row above from lane 4j - 1, which is one column ahead in pair k + 1
            // already; lane 0 takes it from the stripe above, whose last lane went through the same virtual columns; only the
            // diagonal of the first column (upH_prev) comes from the reset.  A lane that still is in pair k reads a reset
            // neighbour's zero levels: nothing that could raise a maximum either.
            auto reset_lanes = [&](int k, int j) {
                if constexpr (kChain) {
                    int t = tid;
                    asm volatile("" : "+v"(t));   // (addresses rebuilt here, as in block_end)
                    const int ln = t & (LANES - 1), grp = t / LANES;
                    if ((ln >> 2) == j) {
                        u32 m = A::true_of(st.maxv[0], zw[1]);
#pragma unroll
                        for (int d = 1; d < P + 3; d++) m = A::true_max(m, A::true_of(st.maxv[d], zw[d + 1]));
                        u32* const pm = p.scratch + (size_t)gridDim.x * kGroups * (size_t)group_region_words<LANES>(p.lcap) +
                                        ((size_t)blockIdx.x * kGroups + grp) * kChainMaxWords + kGroup * k + ln;
                        if (!first) m = A::true_max(m, *pm);
                        *pm = m;
#pragma unroll
                        for (int d = 0; d < P + 3; d++) st.maxv[d] = zw[d + 1];
#pragma unroll
                        for (int r = 0; r < R; r++) { st.H[r] = zw[r % P]; st.E[r] = zw[r % P + 1]; }
                        st.upH_prev = A::gap(zw[(R - 1) % P], p.gex); st.Hlast = zw[(R - 1) % P]; st.Fout = zw[0];
                    }
                }
            };
            if constexpr (!MULTI) {
                for (int q = 0; q < nquads; q++) quad(q);
            } else if constexpr (kChain) {
                // block by block as below; the quad loop stops where lanes are handed over (wave-uniform scalars)
                constexpr int kNever = 0x7fffffff;
                const int* const ends = chainEnd + (tid >> 6) * kChainMax;
                int rk = 0, rj = 0;
                int nextReset = cnt > 1 ? __builtin_amdgcn_readfirstlane((ends[0] >> 2) + 1) : kNever;
                for (int q0 = 0; q0 < nquads; q0 += BD::kQuadsPerBlock) {
                    const int qend = min(nquads, q0 + BD::kQuadsPerBlock);
                    int q = q0;
                    for (;;) {
                        const int seg = min(qend, nextReset);
                        for (; q < seg; q++) quad(q);
                        if (q >= qend) break;
                        reset_lanes(rk, rj);   // q == nextReset: before quad q
                        nextReset++;
                        if (++rj == 4) {
                            rj = 0;
                            rk++;
                            nextReset = rk + 1 < cnt ? __builtin_amdgcn_readfirstlane((ends[rk] >> 2) + 1) : kNever;
                        }
                    }
                    if (qend == q0 + BD::kQuadsPerBlock) block_end(q0 / BD::kQuadsPerBlock);
                }
            } else {
                // multi-stripe: block by block (Border<LANES>: kQuadsPerBlock quads, then the block transfer)
                for (int q0 = 0; q0 < nquads; q0 += BD::kQuadsPerBlock) {
                    const int qend = min(nquads, q0 + BD::kQuadsPerBlock);
                    for (int q = q0; q < qend; q++) quad(q);
                    if (qend == q0 + BD::kQuadsPerBlock) block_end(q0 / BD::kQuadsPerBlock);
                }
            }
            if constexpr (MULTI) {
                // The last lane has emitted positions 0 .. 4*nquads - 1; the next stripe's lane 0 reads positions up to
                // 4*nquads + LANES - 2 (its columns up to 4*nquads - 1): LANES pairs of "no value" (the kind's unraised zero
                // pattern) go behind the last emitted one — into the OUT ring where they fall into the partial block, straight
                // to the scratch where they fall into the block behind it — and the partial block leaves the OUT ring.
                if (!last) {
                    const int done = nquads & ~(BD::kQuadsPerBlock - 1);           // quads in complete (flushed) blocks
                    const int slot = 4 * (nquads - done) + lane;                     // this lane's "no value" pair: position 4 * done + slot
                    u32* const g = gBorder + (size_t)(done / BD::kQuadsPerBlock) * BD::kBlockWords;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    if (slot < BD::kBlockCols) *reinterpret_cast<uint2*>(ringOut + 8 * slot) = make_uint2(A::kZero, A::kZero);
                    else *reinterpret_cast<uint2*>(g + 2 * slot) = make_uint2(A::kZero, A::kZero);   // in the block behind: the flush below does not touch it
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    *reinterpret_cast<uint4*>(g + 4 * lane) = *reinterpret_cast<const uint4*>(ringOut + 16 * lane);
                }
            }
            if constexpr (kUni) {
                // accumulator d and zero level zw[d + 1] (the window of quad nquads) are in the same frame -> true scores
                // (a chain's window was seeded without the stripes above at its last border)
                const u32 above = maxv;
                maxv = A::true_of(st.maxv[0], zw[1]);
#pragma unroll
                for (int d = 1; d < P + 3; d++) maxv = A::true_max(maxv, A::true_of(st.maxv[d], zw[d + 1]));
                if constexpr (kChain) {
                    if (cnt > 1) maxv = A::true_max(maxv, above);
                }
            } else if constexpr (OFFS) {
                if constexpr (A::kWindow) {
                    // accumulator d and zero level d are in the same frame -> true scores
                    maxv = A::true_of(st.maxv[0], st.Zc[0]);
#pragma unroll
                    for (int d = 1; d < P + 3; d++) maxv = A::true_max(maxv, A::true_of(st.maxv[d], st.Zc[d]));
                } else {
                    // Zc[c + 1] is the NEXT column's level of class c + 1: 2a above the accumulator's frame
                    maxv = A::true_of(st.maxv[0], A::gap(A::gap(st.Zc[1], p.gex), p.gex));
#pragma unroll
                    for (int c = 1; c < P; c++)
                        maxv = A::true_max(maxv, A::true_of(st.maxv[c], A::gap(A::gap(st.Zc[c + 1], p.gex), p.gex)));
                }
            } else {
                maxv = st.maxv[0];
            }
            if constexpr (MULTI) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        }

        // a pair's scores from the lanes' maxima (true scores): nq the quads of its walk, col0 its first column in the walk
        // (a chain's virtual subject; else 0)
        auto finish = [&](bool valid0, bool valid1, int pos0, int pos1, u32 maxv, int nq, int col0) {
            int sc0, sc1, guard = 0;
            if constexpr (OFFS) {
                // group maximum of true scores
                if constexpr (LANES == 8) {
                    maxv = half_row_max(maxv, [](u32 a, u32 b) { return A::true_max(a, b); });
                } else if constexpr (LANES == 4) {
                    maxv = quad_max(maxv, [](u32 a, u32 b) { return A::true_max(a, b); });
                } else {
                    maxv = row_max_true<KIND>(maxv);
                }
                if constexpr (LANES == 64) {
                    maxv = A::true_max(maxv, (u32)__shfl_xor((int)maxv, 16));
                    maxv = A::true_max(maxv, (u32)__shfl_xor((int)maxv, 32));
                }
                sc0 = A::true_lo(maxv);
                sc1 = A::true_hi(maxv);
                // no value of the alignment exceeded score + its cell's zero level: inside the exact range below the limit.  Column
                // frame: a * (columns + 2 LANES + ...); uniform frame: a * (t_g + P + ...), t_g < 4 nquads + LANES (nstripes - 1) or K
                if constexpr (kUni) {
                    // (and never less than the column frame would: the same subjects are flagged and re-scored wherever that
                    // bound is the larger one — in practice everywhere but short subjects of queries of many stripes)
                    const int tgmax = 4 * nq + col0 + LANES * (p.nstripes - 1);
                    constexpr int kColP = frame_classes(true, R, LANES, MULTI);
                    guard = max(p.gex_mag * ((tgmax > 4 * rq ? 4 * rq : tgmax) + P + 8),
                                p.gex_mag * (min(4 * nq, p.flag_period) + 2 * LANES + 4 + kColP));
                } else {
                    guard = p.gex_mag * (4 * nq + 2 * LANES + 4 + P);
                }
            } else {
                maxv = group_max<KIND, LANES>(maxv);
                sc0 = A::score_lo(maxv);   // (32-bit kinds: one subject per group)
                sc1 = 0;
            }
            if (lane == 0) {
                if (valid0) {
                    if (A::kPacked && p.ovf_check && sc0 >= A::kLimit - guard) {
                        __hip_atomic_store(p.ovf_pos + atomicAdd(p.ovf_count, 1), pos0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    } else {
                        p.scores[pos0] = (float)sc0;
                        if (p.stat_count && sc0 >= p.stat_limit) atomicAdd(p.stat_count, 1);
                    }
                    p.ids[pos0] = (int32_t)(p.id_offset + pos0);
                }
                if (valid1) {
                    if (p.ovf_check && sc1 >= A::kLimit - guard) {
                        __hip_atomic_store(p.ovf_pos + atomicAdd(p.ovf_count, 1), pos1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    } else {
                        p.scores[pos1] = (float)sc1;
                    }
                    p.ids[pos1] = (int32_t)(p.id_offset + pos1);
                }
            }
        };
        if constexpr (kChain) {
            int col0 = 0;
            for (int k = 0; k < cnt; k++) {
                const Pair q = load_pair(hb + k);
                const int lm = __builtin_amdgcn_readfirstlane(q.lmax);
                const bool lastPair = k + 1 == cnt;
                int t = tid;
                asm volatile("" : "+v"(t));
                const u32* const pm = p.scratch + (size_t)gridDim.x * kGroups * (size_t)group_region_words<LANES>(p.lcap) +
                                      ((size_t)blockIdx.x * kGroups + t / LANES) * kChainMaxWords + kGroup * k + (t & (LANES - 1));
                u32 m = maxv;
                if (!lastPair) m = *pm;
                // (the early-flag bound of a pair from its own columns; the last pair's walk is what is left of the chain's)
                finish(q.valid0, q.valid1, q.pos0, q.pos1, m, lastPair ? nquads - col0 / 4 : (lm + LANES - 1 + 3) >> 2, col0);
                col0 += chain_pair_columns(lm) + 4;
            }
        } else {
            finish(valid0, valid1, pos0, pos1, maxv, nquads, 0);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Profile builder: tile[stripe][letter][chunk][lane][4 words] from the encoded query and the matrix.
// Replaces the per-block pair-table construction of the reference (half2_kernels.cuh:57-65).
//
// Score source: the substitution table, indexed by the query's letters — or, when `query` is null, a position-specific
// scoring matrix in its staged form (sw_pssm.hpp), indexed by the query POSITION; matrix21 then points to the staged PSSM
// and pad_row to its first padding row (= qlen).  Everything behind the score (layout, frame terms, wide words) is shared.
// ------------------------------------------------------------------------------------------------
template <int KIND, int R, int LANES>
__global__ void sw_build_profile_kernel(const int8_t* __restrict__ query, int32_t qlen,
                                        const int8_t* __restrict__ matrix21, int32_t pad_row, int32_t nstripes,
                                        unsigned char* __restrict__ profile, int32_t shift, int32_t head_extra) {
    using A = Arith<KIND>;
    using G = Geometry<KIND, R, LANES>;
    constexpr int kWordsPerRow = G::kRowBytes / 4;
    constexpr int kWordsPerChunkRow = G::kChunkRowBytes / 4;
    const size_t total = (size_t)nstripes * kLetters * kWordsPerRow;
    u32* out = reinterpret_cast<u32*>(profile);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int word = (int)(i % kWordsPerRow);
        const int letter = (int)((i / kWordsPerRow) % kLetters);
        const int stripe = (int)(i / ((size_t)kWordsPerRow * kLetters));
        const int chunk = word / kWordsPerChunkRow, lane = ((word % kWordsPerChunkRow) / 4) % LANES, sub = word % 4;
        const int w = G::C::first(chunk) + sub;  // word index within the lane's NW words (Chunks: 4- and 3-word chunks)
        u32 v = 0;
        if (sub < G::C::words(chunk) && w < G::NW) {
            auto entry = [&](int row_in_lane) -> u32 {
                if (row_in_lane >= R) return 0u;  // unused upper half of an odd R's last word
                const int64_t row = (int64_t)stripe * G::kStripeRows + lane * R + row_in_lane;
                // matrix21: (query letters + one padding row `pad_row`) x 21 subject letters
                const bool pssm = query == nullptr;
                const int qc = row < qlen ? (pssm ? (int)row : (int)query[row]) : pad_row;
                const int score = pssm ? (int)matrix21[pssm_index(qc, letter)] : (int)matrix21[qc * kLetters + letter];
                // OFFS kernels (shift = a): the diagonal step raises the frame by a per column and by a per row class;
                // the row above lane-local row 0 is the previous lane's last row (dp_step<OFFS>), whose frame lies a further
                // a * head_extra below in the uniform frame (sw_scan_kernel; head_extra = 1; the column frame: 0)
                const int P = frame_classes(A::kPacked, R, LANES, nstripes > 1, head_extra != 0);  // the scan kernel's (MULTI == more than one stripe)
                const int cls = row_in_lane % P, above = (row_in_lane == 0 ? R - 1 : row_in_lane - 1) % P;
                const int head = row_in_lane == 0 ? head_extra : 0;
                return A::encode_score(score + shift * (1 + head + cls - above));
            };
            if constexpr (G::kWide) v = w < R ? (entry(w) | (A::kOne << 16)) : 0u;
            else if constexpr (A::kPacked) v = entry(2 * w) | (entry(2 * w + 1) << 16);
            else v = entry(w);
        }
        out[i] = v;
    }
}

}  // namespace swk
