// sw_api.hip — the scan path of the C ABI declared in include/cudasw4_amd.h.
//
// Host-side glue only: context state (matrix, query, per-kind profile), the launch plan (sw_plan.hpp: query plan, group
// shape, frame, streamed rounds, pair chains, grid and scratch — decided once by plan_launch and read by the sizing, the
// reporting and the launching entry points alike), the scan and overflow re-score launches and the row-pipeline entry
// points.  Top-K lives in sw_topk.hip, the probes and micro-runs in sw_probe.hip, the context itself in sw_ctx.hpp.
// There is NO CPU fallback anywhere: without a HIP device every entry point fails with SW_ERR_NO_DEVICE/SW_ERR_HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/cudasw4_amd.h"
#include "../../include/cudasw4_amd_engine.h"
#include "../../include/cudasw4_amd_pssm.h"
#include "sw_ctx.hpp"
#include "sw_launch.hpp"
#include "sw_pssm.hpp"
#include "sw_rows_pipeline.hpp"

using swi::fail;
using swi::kWorkSlots;
using swi::Profile;
using swp::LaunchPlan;
using swp::LaunchRequest;
using swp::PlanSettings;

namespace {

thread_local std::string g_last_error = "";

const swk::KindLaunch* kind_launch(int kind) {
    switch (kind) {
        case SW_KIND_F16X2: return &swk::launch_f16x2();
        case SW_KIND_I16X2: return &swk::launch_i16x2();
        case SW_KIND_I32: return &swk::launch_i32();
        case SW_KIND_F32: return &swk::launch_f32();
    }
    return nullptr;
}

bool kind_packed(int kind) { return kind == SW_KIND_F16X2 || kind == SW_KIND_I16X2; }

struct QueryPlan {
    int rows = 0;      // R: query rows per lane
    int nstripes = 0;  // stripes of lanes*R rows
    int lanes = 16;    // lanes per alignment group: 16 (DPP row), 64 (whole wave, long subjects) or 8 (half row, short queries)
};

// Pick (R, nstripes) with R a compiled value.  Replaces the reference's subject-length ->
// (group_size, numRegs) table (cudasw4.cuh:1764-1912); here the tile shape follows the QUERY length
// because the query is the register-resident dimension, and the subject length only selects the group
// width: 16 lanes for the bulk of a DB, the whole wave for the long partitions 34/35.
// Cost model: a step of a stripe with R rows per lane issues ~(R + 1.2) row-equivalents of VALU work
// (per-step DPP/address overhead) and every stripe pays its own pipeline fill; minimise ns * (R + 1.2).
QueryPlan plan_query(int kind, int32_t qlen, int lanes) {
    const swk::KindLaunch* kl = kind_launch(kind);
    QueryPlan pl;
    pl.lanes = lanes;
    if (!kl || qlen <= 0) return pl;
    const int maxrows = swk::max_rows(kind, lanes);
    // fp32 multi-stripe kernels above 32 rows per lane lose the third wave per SIMD (their single-stripe kernels keep it up to 36)
    const int maxrows_multi = (kind == SW_KIND_F32 && lanes <= 16) ? std::min(maxrows, swk::kMaxRowsScalarMulti) : maxrows;
    // packed kinds: a multi-stripe kernel above kWaves3MaxRowsPackedMulti rows per lane holds two waves per SIMD, which
    // fill 93.5 % of the issue slots at best (three: 97+ %).  Measured on the peak DB, the same queries with 32-row stripes
    // at three waves against 40..47-row stripes at two (tools/variant_bench2.sh): a step-row of the tall kernels costs
    // 5 % more (fitted together with the per-step overhead below on ten queries of 1500..5478 residues).  CUDASW4_AMD_TWO_WAVE_PENALTY overrides the factor (1: the planner of rounds 1-3; tests use it to reach
    // every compiled shape).
    double two_wave_penalty = 1.05;
    if (const char* e = getenv("CUDASW4_AMD_TWO_WAVE_PENALTY")) two_wave_penalty = std::max(1.0, atof(e));
    const bool has_three_wave_multi = kl->packed && lanes <= 16 && swk::kWaves3MaxRowsPackedMulti > maxrows / 2;
    double best = 1e300;
    auto consider = [&](int ns) {
        const int64_t per_lane = (qlen + (int64_t)lanes * ns - 1) / ((int64_t)lanes * ns);
        int r = (int)((per_lane + swk::kRowsGranule - 1) / swk::kRowsGranule * swk::kRowsGranule);
        r = std::max(r, swk::kRowsGranule);
        if (r > (ns > 1 ? maxrows_multi : maxrows)) return;
        if (ns > 1 && 2 * r <= maxrows) return;  // multi-stripe kernels exist for R > max/2 only
        // per-step overhead in row equivalents: ~10 VALU ops single-stripe; with several stripes ~20 with the stripe border,
        // plus the tile load and the two barriers of every stripe switch spread over the stripe's steps
        double cost = ns * (r + (ns > 1 ? 3.0 : 1.2));
        if (has_three_wave_multi && ns > 1 && r > swk::kWaves3MaxRowsPackedMulti) cost *= two_wave_penalty;
        if (cost < best - 1e-9) { best = cost; pl.rows = r; pl.nstripes = ns; }
    };
    if (qlen <= (int64_t)lanes * maxrows) consider(1);
    const int64_t stripe_multi = (int64_t)lanes * maxrows_multi;
    const int ns_m = std::max<int>(2, (int)((qlen + stripe_multi - 1) / stripe_multi));
    int ns_hi = ns_m + 2;
    if (has_three_wave_multi) {  // ... and the plans on three-wave stripes
        const int64_t stripe3 = (int64_t)lanes * swk::kWaves3MaxRowsPackedMulti;
        ns_hi = std::max<int>(ns_hi, (int)((qlen + stripe3 - 1) / stripe3) + 1);
    }
    for (int ns = ns_m; ns <= ns_hi; ns++) consider(ns);
    return pl;
}

}  // namespace

// Longest query that runs on 8-lane groups.  Tuned on RAGGED subjects (tools/ragged_query_sweep.py, Swiss-Prot-like DB
// through the C++ driver): the packed kinds gain 2.4 ... 7.3 % up to 256 residues (R = 32: still three waves per SIMD)
// and nothing consistent above (272: -1 %, 288: +1.5 %, 304: -3 %); the 32-bit kinds gain 4 ... 14 % up to 256 (R = 32:
// the last height at which their single-stripe kernels keep three waves per SIMD without spills) and lose from 272 on,
// so both limits are 256 (the 32-bit limit stood at 240 until round 4, below what the sweep supports).  (Round 2 tuned on the peak DB, whose identical subjects hid the LDS bank conflicts of the second group
// of a DPP row — fixed since, Geometry / dp_step: laneStep — and chose 288 / 240: +14 % at 144 residues there.)
#ifndef SW_LANES8_MAX_QUERY_PACKED
#define SW_LANES8_MAX_QUERY_PACKED 256
#endif
#ifndef SW_LANES4_MAX_QUERY_PACKED
#define SW_LANES4_MAX_QUERY_PACKED 96
#endif
#ifndef SW_LANES4_MAX_QUERY_SCALAR
#define SW_LANES4_MAX_QUERY_SCALAR 128
#endif
#ifndef SW_LANES4_MAX_SUBJECT
#define SW_LANES4_MAX_SUBJECT 1280
#endif
#ifndef SW_LANES4_MIN_BATCHES_PER_CU
#define SW_LANES4_MIN_BATCHES_PER_CU 12
#endif
#ifndef SW_LANES8_MAX_SUBJECT
#define SW_LANES8_MAX_SUBJECT 192
#endif
#ifndef SW_LANES8_MAX_QUERY_SCALAR
#define SW_LANES8_MAX_QUERY_SCALAR 256
#endif

namespace {

// The largest score one aligned pair of residues can add: every bound that is derived from "a score cannot exceed
// (aligned columns) x (largest substitution score)" reads PlanSettings::score_max, so that a PSSM query is bounded by its
// own entries and not by a table it never uses.  Refreshed whenever the matrix, the query or its kind changes.
void refresh_score_max(sw_ctx* ctx) { ctx->plan.score_max = std::max(1, ctx->pssm_mode ? ctx->pssm_max : ctx->matrix_max); }
// something to score with: a substitution table for a letter query; a PSSM query brings its own scores
bool have_scores(const sw_ctx* ctx) { return ctx->have_matrix || ctx->pssm_mode; }

int max_grid(const PlanSettings& s) {
    const int g = std::max(1, s.num_cus) * s.grid_mult;
    return s.grid_cap > 0 ? std::min(g, s.grid_cap) : g;
}

// Reference partitions 34 (1281..8000) and 35 (> 8000) hold the long subjects.  When there are only a few
// of them (the tail of a real DB) they get the wave-wide group shape: 4x the lanes per alignment, so the
// giants finish 4x sooner.  When the partition alone can fill the GPU several times (e.g. the L=2048
// peak DB) the 16-lane shape is more efficient (more rows per lane, less per-step overhead, wide profile words).
// Partition 34 takes the 16-lane shape already from 512 subjects up: in a Swiss-Prot-like DB it holds 2.4 % of the
// sequences but 11 % of the residues, its launch runs next to the bulk launch on a side stream, and a subject of at
// most 8000 residues is no tail there (Swiss-Prot-like DB: 10.7 -> 11.05 TCUPS).
// overflowed subjects can have any length: long ones would dominate a 16-lane launch
int rescore_lanes(int32_t max_subject_len) { return max_subject_len > 1280 ? 64 : 16; }

int shape_index(int lanes) { return lanes == 64 ? 1 : lanes == 8 ? 2 : lanes == 4 ? 3 : 0; }

// The int32 kind in fp32 lanes.  On gfx950 the fp32 form of the recurrence runs 30 % faster than the int32 form (8.35
// against 6.44 TCUPS on the peak DB): v_add_f32 co-issues with v_max3_f32, v_add_u32 does not.  fp32
// arithmetic on integers is exact below 2^24, a score cannot exceed min(query, subject) * (largest substitution score),
// and the column-offset frame raises values by at most 2^22 (scan_common: `room`) — so whenever that bound stays below
// 2^24 the int32 launch is served by the fp32 kernels with bit-identical results (they are written as floats either way,
// like the reference's BatchResultList).  Anything beyond the bound, e.g. a 2-million-residue query against a subject
// of the same size, gets the true int32 kernels.
int effective_kind_of(const PlanSettings& s, int kind, int32_t max_subject_len) {
    if (kind != SW_KIND_I32 || s.i32_native || !s.have_query) return kind;
    const int64_t bound = (int64_t)std::min(s.qlen, max_subject_len) * s.score_max + ((int64_t)1 << 22) + 4096;
    return bound < ((int64_t)1 << 24) ? SW_KIND_F32 : SW_KIND_I32;
}

// Short queries run on 8-lane groups (half DPP rows): twice the rows per lane for the same query, so the per-step
// overhead is spread over twice the cells, and 7 instead of 15 fill steps per subject (sw_dp_kernel.hpp: Shift).
int lanes_for_partition_any(const PlanSettings& s, int kind, int part_id, int32_t n, int32_t max_subject_len);
int lanes_for_partition(const PlanSettings& s, int kind, int part_id, int32_t n, int32_t max_subject_len) {
    const int lanes = lanes_for_partition_any(s, kind, part_id, n, max_subject_len);
    // the streamed packed kernels (16-lane groups) keep a slot's lengths in 16 bits: subjects beyond that — thousands of
    // them in one packed launch, or a caller that forces the shape — take the wave-wide groups
    return (lanes == 16 && kind_packed(kind) && max_subject_len >= 0xffff) ? 64 : lanes;
}
int lanes_for_partition_any(const PlanSettings& s, int kind, int part_id, int32_t n, int32_t max_subject_len) {
    if (part_id < SW_NUM_LENGTH_PARTITIONS - 2) {
        if (!s.have_query) return 16;
        // very short queries: 4-lane groups (a DPP quad; single-stripe kernels only).  A batch is 128 (packed kinds) or 64
        // subjects then: only where the launch still hands every workgroup slot several batches
        const int32_t limit4 = s.lanes4_max_q >= 0 ? s.lanes4_max_q : kind_packed(kind) ? SW_LANES4_MAX_QUERY_PACKED : SW_LANES4_MAX_QUERY_SCALAR;
        const int64_t batches4 = (int64_t)n / (64 * (kind_packed(kind) ? 2 : 1));
        const bool enough4 = s.lanes4_max_q >= 0 || batches4 >= (int64_t)SW_LANES4_MIN_BATCHES_PER_CU * std::max(1, s.num_cus);   // (an explicit limit: tests reach the shape with a handful of subjects)
        // ... and holds no long subject: a column costs a quad ~(6.5 R + 19) instructions with R = a quarter of the query, and
        // the longest subject's walk bounds the launch (partition 34 merged into a 96-residue query's launch: 3.6 ms
        // against 1.8 ms of instructions); the host driver keeps partition 34 out of such a launch
        const int32_t lmax4 = s.lanes4_max_subject >= 0 ? s.lanes4_max_subject : SW_LANES4_MAX_SUBJECT;
        if (s.qlen <= 4 * swk::max_rows(kind, 4) && s.qlen <= limit4 && enough4 && max_subject_len <= lmax4) return 4;
        const bool fits8 = s.qlen <= 8 * swk::max_rows(kind, 8);  // one stripe of 8-lane groups
        const int32_t limit = s.lanes8_max_q >= 0 ? s.lanes8_max_q : kind_packed(kind) ? SW_LANES8_MAX_QUERY_PACKED : SW_LANES8_MAX_QUERY_SCALAR;
        if (fits8 && s.qlen <= limit) return 8;
        // (rounds 2-5 ran multi-stripe queries on SHORT subjects — up to 192 residues — on 8-lane groups: twice the stripes, each
        // filling its pipeline in 7 instead of 15 steps, +2.5 % at L = 128.  The streamed 16-lane kernels pay the fill once per
        // round of up to 16 subject pairs: 10 931 against 10 537 GCUPS for the 1000-residue query at L = 128.)
        return 16;
    }
    const int64_t fills_gpu_twice = (int64_t)2 * std::max(1, s.num_cus) * 4 * 32;
    if (part_id == SW_NUM_LENGTH_PARTITIONS - 2) return n >= (s.long16_min >= 0 ? s.long16_min : 512) ? 16 : 64;
    return n >= fills_gpu_twice ? 16 : 64;
}


// The profile of the plan's (kind, group shape, frame), built on `stream` unless the context holds it already.
// frame: 0 plain recurrence, 1 column frame, 2 uniform frame (swk::uniform_frame_launch: row 0's profile entries a higher)
int ensure_profile(sw_ctx* ctx, const LaunchPlan& lp, int shift, hipStream_t stream) {
    Profile& pr = ctx->profiles[lp.kind][shape_index(lp.lanes)][lp.frame];
    // other gap-extension score than last time, or other stripes (CUDASW4_AMD_TWO_WAVE_PENALTY changed under a live query)
    if (pr.valid && (pr.shift != shift || pr.rows != lp.rows || pr.nstripes != lp.nstripes)) pr.valid = false;
    if (pr.valid) {
        // built on another stream earlier in this query: order this stream after the build
        SW_HIP(hipStreamWaitEvent(stream, pr.ready, 0));
        return SW_OK;
    }
    const swk::KindLaunch* kl = kind_launch(lp.kind);
    const int32_t qlen = ctx->plan.qlen;
    const size_t bytes = kl->tile_bytes(lp.rows, lp.lanes) * (size_t)lp.nstripes;
    if (bytes == 0) return fail(SW_ERR_INVALID, "no kernel compiled for this query plan");
    if (bytes > pr.capacity) {
        // hipFree/hipMalloc synchronise the device: they would serialise launches that are meant to overlap
        // on other streams, so capacity starts at 2 MiB (queries up to ~50 k residues) and doubles
        const size_t cap = std::max<size_t>(std::max(bytes, 2 * pr.capacity), size_t(2) << 20);
        if (pr.dev) SW_HIP(hipFree(pr.dev));
        pr.dev = nullptr;
        pr.capacity = 0;
        SW_HIP(hipMalloc(&pr.dev, cap));
        pr.capacity = cap;
    }
    // (a null query selects the builder's PSSM source: scores by query position from the staged PSSM, padding row = qlen)
    if (ctx->pssm_mode) SW_HIP(kl->profile(lp.rows, lp.lanes, nullptr, qlen, ctx->d_pssm, qlen, lp.nstripes, pr.dev, shift, lp.frame == 2 ? 1 : 0, stream));
    else SW_HIP(kl->profile(lp.rows, lp.lanes, ctx->d_query, qlen, ctx->d_matrix, ctx->dim, lp.nstripes, pr.dev, shift, lp.frame == 2 ? 1 : 0, stream));
    pr.shift = shift;
    if (!pr.ready) SW_HIP(hipEventCreateWithFlags(&pr.ready, hipEventDisableTiming));
    SW_HIP(hipEventRecord(pr.ready, stream));
    pr.rows = lp.rows;
    pr.nstripes = lp.nstripes;
    pr.valid = true;
    return SW_OK;
}

// scratch words per (workgroup, group) array for subjects up to max_len
int32_t border_capacity(int32_t max_len, int lanes) {
    const int64_t steps = ((int64_t)max_len + lanes - 1 + 3) / 4 * 4;
    return (int32_t)((steps + 15) / 16 * 16 + 16);  // + one prefetched quad past the end, rounded to 64 bytes
}
size_t border_bytes_per_wg(int32_t lcap, int lanes) {
    if (lanes == 4) return 0;   // single-stripe kernels only: no border
    // (16-lane groups: the border array and, behind it, the address stream of the packed sw_scan_kernel — 8 + 4 bytes per column)
    const size_t region = lanes == 16 ? swk::group_region_words<16>(lcap) : lanes == 8 ? swk::group_region_words<8>(lcap) : swk::group_region_words<64>(lcap);
    return (size_t)(swk::kThreads / lanes) * region * sizeof(uint32_t);
}

// Pair chains (sw_dp_kernel.hpp): the batches a claim of a launch takes.  Only the packed multi-stripe sw_scan_kernel on
// 16-lane groups chains (plain ranges, one pair at a time: stream_slots == 1), and a launch of so few batches that none of
// its claims would be a chain (the kernel's tail rule: more than chain * grid batches must remain) keeps today's scratch.
// Measured at two points only (profiles/pair_chain_results.md): 5 batches per workgroup lose 0.6 % with chains of 3, 40 gain
// 1.2 %; the threshold lies where the expected gain (1.3 % of the chained rounds) is about three times the loss seen at 5.
constexpr int kChainMinRounds = 16;
// Not measured: a chained border saves about 10 steps of a pair's walk (under 1 % from 1024 columns on), and the scratch
// grows with the chain's columns.
constexpr int32_t kChainMaxSubject = 1024;
int chain_wanted(const PlanSettings& s, int kind, int lanes, bool multi, int stream_slots, int64_t nbatches, int32_t max_subject_len) {
    if (!kind_packed(kind) || lanes != 16 || !multi || stream_slots != 1) return 1;
    if (s.chain <= 1 || max_subject_len > kChainMaxSubject) return 1;
    // ... and so does a launch of at most kChainMinRounds batches per workgroup: chained workgroups leave the lock-step of
    // equal batches, which costs the end of a launch a fraction of a batch's walk, more than 1.3 % of a few rounds bring
    // (125 000 subjects of 512 residues, 5 rounds: -0.6 % with chains of 3; profiles/pair_chain_results.md)
    if (!s.chain_all && nbatches <= (int64_t)std::max(s.chain, kChainMinRounds) * max_grid(s)) return 1;
    return std::min<int>(s.chain, swk::kChainMax);
}
// the border capacity of a chain's virtual subject, and a workgroup's scratch with it: the regions and the per-pair maxima
int32_t chain_capacity(int32_t max_len, int chain, int lanes) {
    return border_capacity((int32_t)std::min<int64_t>(swk::chain_columns(max_len, chain), SW_MAX_SUBJECT_LEN), lanes);
}
size_t chain_bytes_per_wg(int32_t max_len, int chain, int lanes) {
    if (chain <= 1) return border_bytes_per_wg(border_capacity(max_len, lanes), lanes);
    return border_bytes_per_wg(chain_capacity(max_len, chain, lanes), lanes) + (size_t)(swk::kThreads / lanes) * swk::kChainMaxWords * sizeof(uint32_t);
}

// Debug check of the max_subject_len contract (include/cudasw4_amd.h): longest subject of the range / of the listed positions
__global__ void max_length_kernel(const int32_t* lengths, const int32_t* positions, const int32_t* count_ptr, int32_t first_pos,
                                  int32_t n, int32_t* out) {
    const int32_t cnt = count_ptr ? min(*count_ptr, n) : n;
    int32_t m = 0;
    for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x)
        m = max(m, lengths[positions ? positions[i] : first_pos + i]);
    if (m > 0) atomicMax(out, m);
}

// Streamed subjects (sw_stream_kernel.hpp).  The levels of a round start at `base` and rise by a per column and by `jump` per
// slot border; a subject is exact while level + score stays inside the kind's exact range, so the round's a * columns + jumps
// may add up to `room`: what is left between the base and the highest level at which unrelated subjects (and moderate hits)
// still pass unflagged.
//   fp16: exact integers in [-2048, 2048]: base -2016, levels up to 1024 (a subject in the last columns of a round is flagged
//         from 2048 - 1024 on — round 5's frame flagged from 988 on everywhere), jump 128;
//   int16: biased patterns exact up to 31 743, limit 25 000: base 0, levels up to 12 400, jump 512.
// A slot whose predecessor scored jump - 4 or more is re-scored (its lanes may have kept values above the raised levels):
// the jump is what separates "unrelated" from "a hit" — 128 is far above the noise floor of a 35 000-residue subject (~90).
struct StreamPlan { int slots = 0, cols = 0, room = 0, base = 0, jump = 0; };
StreamPlan stream_plan(const PlanSettings& s, int kind, int lanes, int a, const QueryPlan& pl, int32_t max_subject_len) {
    StreamPlan sp;
    if (!kind_packed(kind) || lanes != 16 || a < 0) return sp;   // (a < 0: offs_possible sends the launch to the 32-bit kind)
    const bool multi = pl.nstripes > 1;
    const int P = swk::frame_classes(true, pl.rows, lanes, multi);
    sp.base = kind == SW_KIND_F16X2 ? -2016 : 0;
    const int top = kind == SW_KIND_F16X2 ? 1024 : 12400;
    sp.jump = s.stream_jump > 0 ? s.stream_jump : (kind == SW_KIND_F16X2 ? 512 : 2048);
    sp.room = top - sp.base - a * (2 * lanes + 4 + P);
    sp.cols = a > 0 ? std::min(sp.room / a, s.stream_cols_max) : s.stream_cols_max;   // (a = 0: the levels do not grow)
    sp.slots = std::max(1, std::min(s.stream_slots, swk::kStreamMaxSlots));
    // a gap-extension score so large that not even two short slots fit a round: one slot at a time
    if (sp.room < 4 * lanes * a || sp.cols < 4 * lanes) sp.slots = 1;
    // Several stripes: a slot border costs the streamed kernels about seven step equivalents per stripe (the separator column,
    // sixteen steps of a second copy of the loop body, two transitions between the copies' register allocations) against the
    // sixteen of a pipeline drain and the rounding to whole quads — worth it while the subjects are short (measured, peak DB,
    // 1000- / 5478-residue queries: L = 128 +3.7 / +1.1 % over round 5's 8-lane groups, L = 256 +0.7 / +0.6 %, L = 512
    // +0.1 / -1.5 %; int16, whose rounds are longer: L = 256 -0.1 / -3.8 %, L = 512 -0.9 / -5.5 %), and with rounds whose
    // border arrays stay small.  Longer subjects: sw_scan_kernel, one pair at a time (slots = 1 selects it, sw_launch.hpp).
    if (multi) {
        // (measured with rounds of up to 1 536 columns, against sw_scan_kernel on 16-lane groups: fp16 L = 128 +4.5 / +2.8 %,
        // L = 256 +3.0 / +0.7 %, L = 512 +0.7 / -0.1 %; int16 L = 128 +4.2 / +2.0 %, L = 256 -0.4 / -0.4 %, L = 512 -0.7 / -1.6 %:
        // profiles/r06_stream_ab.txt)
        const int32_t limit = s.stream_multi_max_subject >= 0 ? s.stream_multi_max_subject : (kind == SW_KIND_F16X2 ? 320 : 192);
        if (max_subject_len > limit) sp.slots = 1;
        sp.cols = std::min(sp.cols, s.stream_multi_cols_max);
    }
    return sp;
}

// The column-offset recurrence needs (i) a frame period K of at least 4 * lanes columns inside the kind's room — the
// longest run of columns in one frame plus the pipeline skew: a * (K + 3 * lanes + 16) <= room —, (ii) for a packed kind an
// overflow list to flag into (a subject whose bound score + a * columns reaches the limit is flagged early), (iii) gop - gex
// inside the 16-bit encodings.  *K_out: the period (0: the frame is never lowered).
bool offs_possible(const PlanSettings& s, int kind, int lanes, int32_t max_subject_len, int gop, int gex, int ovf_check, int64_t* K_out) {
    const int a = -gex;
    const int64_t room = kind == SW_KIND_F16X2 ? 1536 : kind == SW_KIND_I16X2 ? 12500 : (int64_t)1 << 22;
    int64_t K = 1 << 21;
    while (K >= 4 * lanes && (int64_t)a * (K + 3 * lanes + 16) > room) K >>= 1;
    // int16: the room would allow a period of 8192 columns, but the flag bound grows with the period (score + a * min(columns,
    // K) + ...): with 8192 a 4000-residue protein was re-scored from 21 000 up instead of 25 000.  2048 columns cost 0.3 % in
    // lowering steps and keep the early flags within 8 % of the limit.
    if (kind == SW_KIND_I16X2) K = std::min<int64_t>(K, std::max<int64_t>(2048, 4 * lanes));
    if (!kind_packed(kind) && max_subject_len + 3 * lanes + 16 > K) K = 0;  // the 32-bit kernels do not lower their frame
    if (K_out) *K_out = K;
    return s.use_offs && K >= 4 * lanes && (!kind_packed(kind) || (ovf_check && a >= 0)) && gop - gex >= -1000;
}
// A packed launch that cannot run the column-offset recurrence is served by its 32-bit kind (exact, nothing to flag): the
// plain form of the packed recurrence is no longer compiled (round 6: it was half of the packed code objects for gap scores
// nobody uses — |gex| > 12 with fp16 — and for callers that pass no overflow list).  CUDASW4_AMD_NO_OFFS=1 takes every
// packed launch there (tests of the fallback).
int packed_fallback_kind(int kind) { return kind == SW_KIND_F16X2 ? SW_KIND_F32 : SW_KIND_I32; }

}  // namespace

// ------------------------------------------------------------------ the launch plan (sw_plan.hpp)
namespace swp {

void settings_from_env(PlanSettings& s) {
    if (const char* e = getenv("CUDASW4_AMD_GRID_CAP")) s.grid_cap = std::max(0, atoi(e));
    if (const char* e = getenv("CUDASW4_AMD_NO_OFFS")) s.use_offs = !(e[0] == '1');
    if (const char* e = getenv("CUDASW4_AMD_I32_NATIVE")) s.i32_native = e[0] == '1';
    if (const char* e = getenv("CUDASW4_AMD_LANES8_MAX_Q")) s.lanes8_max_q = atoi(e);
    if (const char* e = getenv("CUDASW4_AMD_LANES4_MAX_Q")) s.lanes4_max_q = atoi(e);
    if (const char* e = getenv("CUDASW4_AMD_LANES4_MAX_SUBJECT")) s.lanes4_max_subject = atoi(e);
    if (const char* e = getenv("CUDASW4_AMD_STREAM")) s.stream_slots = std::max(0, std::min(swk::kStreamMaxSlots, atoi(e)));
    if (const char* e = getenv("CUDASW4_AMD_CHAIN")) s.chain = std::max(1, std::min(swk::kChainMax, atoi(e)));
    if (const char* e = getenv("CUDASW4_AMD_CHAIN_ALL")) s.chain_all = e[0] == '1';
}

LaunchPlan plan_launch(const PlanSettings& s, const LaunchRequest& req) {
    LaunchPlan lp;
    const int32_t max_len = req.max_subject_len;
    lp.kind = req.kind;
    if (!kind_launch(req.kind)) return lp;
    const bool list = req.part_id < 0;
    auto lanes_of = [&](int kind) { return list ? rescore_lanes(max_len) : lanes_for_partition(s, kind, req.part_id, req.n, max_len); };
    lp.kind = effective_kind_of(s, req.kind, max_len);
    lp.lanes = lanes_of(lp.kind);
    // Column-offset recurrence (7.5 instead of 8.5 instructions per cell pair): values grow by a = -gex per column,
    // so it is used while a * columns leaves room below the kind's limit (offs_possible); a subject whose bound
    // score + a * columns reaches the limit is flagged and re-scored like an overflow.
    int64_t K = 0;
    if (req.gaps_known) {
        lp.offs = offs_possible(s, lp.kind, lp.lanes, max_len, req.gop, req.gex, req.ovf_list, &K);
        if (kind_packed(lp.kind) && !lp.offs) {   // (the 32-bit kind flags nothing: no overflow list)
            lp.fell_back = true;
            lp.kind = effective_kind_of(s, packed_fallback_kind(lp.kind), max_len);
            lp.lanes = lanes_of(lp.kind);
            lp.offs = offs_possible(s, lp.kind, lp.lanes, max_len, req.gop, req.gex, false, &K);
        }
    }
    const int kind = lp.kind, lanes = lp.lanes;
    if (!s.have_query || max_len < 0) return lp;   // (kind and lanes stand; nothing to plan rows, rounds or scratch for)
    lp.valid = true;
    const QueryPlan pl = plan_query(kind, s.qlen, lanes);
    lp.rows = pl.rows;
    lp.nstripes = pl.nstripes;
    lp.multi = pl.nstripes > 1;
    lp.vgpr_slot = pl.rows > 0 ? swk::vgpr_slot_of(kind, pl.rows, lanes, lp.multi) : 0;
    // streamed subjects: plain ranges and lists alike, but never a service launch (32-bit kinds, sized per workgroup)
    const StreamPlan sp = req.service_workgroups > 0 ? StreamPlan() : stream_plan(s, kind, lanes, req.gaps_known ? -req.gex : 1, pl, max_len);
    lp.stream_slots = sp.slots; lp.stream_cols = sp.cols; lp.stream_room = sp.room; lp.stream_base = sp.base; lp.stream_jump = sp.jump;
    // the frame of the kernel that will run (sw_launch.hpp: uniform_frame_launch) selects the profile
    const bool uniform = swk::uniform_frame_launch(kind_packed(kind), lp.offs, lanes, lp.multi, sp.slots);
    lp.frame = lp.offs ? (uniform ? 2 : 1) : 0;
    if (lp.offs) {
        // the uniform frame's period is bounded by its level table (a quarter of a percent of lowering steps at the bound)
        lp.flag_period = K;
        lp.period = uniform ? std::min<int64_t>(K, swk::kUniformMaxPeriod) : K;
    }
    const int subj_per_batch = (swk::kThreads / lanes) * (kind_packed(kind) ? 2 : 1);
    lp.nbatches = std::max<int64_t>(0, ((int64_t)req.n + subj_per_batch - 1) / subj_per_batch);
    int64_t grid = std::min<int64_t>(lp.nbatches, max_grid(s));
    if (req.service_workgroups > 0) grid = std::min<int64_t>(grid, req.service_workgroups);
    if (lp.multi) {
        // what the plan wants: the border arrays of a streamed round hold all of its slots; pair chains (plain ranges
        // only) need regions for the chain's virtual subject and the per-pair maxima
        auto round_capacity = [&](int cols) { return border_capacity(sp.slots > 1 ? std::max(max_len, cols) : max_len, lanes); };
        int cols = sp.cols;
        int chain = (list || req.claim || req.service_workgroups > 0) ? 1 : chain_wanted(s, kind, lanes, true, sp.slots, lp.nbatches, max_len);
        auto per_wg = [&]() { return chain > 1 ? chain_bytes_per_wg(max_len, chain, lanes) : border_bytes_per_wg(round_capacity(cols), lanes); };
        lp.scratch_needed = (size_t)grid * per_wg();
        // what the scratch on offer gives the whole grid: shorter rounds, shorter chains (down to one batch per claim),
        // and at last fewer workgroups
        if (sp.slots > 1) {
            while (cols > max_len && (size_t)grid * per_wg() > req.scratch) cols = cols * 3 / 4;
            lp.stream_cols = cols;
        }
        while (chain > 1 && (size_t)grid * per_wg() > req.scratch) chain--;
        lp.chain = chain;
        lp.lcap = chain > 1 ? chain_capacity(max_len, chain, lanes) : round_capacity(cols);
        lp.bytes_per_wg = per_wg();
        lp.scratch_too_small = req.scratch < lp.bytes_per_wg;
        if (lp.bytes_per_wg > 0) grid = (int64_t)std::min<size_t>((size_t)grid, req.scratch / lp.bytes_per_wg);
    }
    lp.grid = (int)grid;
    // sizing a packed range: the gap scores are not known, and a launch that falls back to its 32-bit kind may need more
    if (!req.gaps_known && kind_packed(req.kind) && !list) {
        LaunchRequest fb = req;
        fb.kind = packed_fallback_kind(req.kind);
        lp.scratch_needed = std::max(lp.scratch_needed, plan_launch(s, fb).scratch_needed);
    }
    return lp;
}

}  // namespace swp

namespace {

// A launch's pair of control words (batch counter of the dynamic batch distribution, counted-in workgroups) from the
// context's ring.  sw_set_query zeroes the next kWorkZeroBlock pairs with ONE memset on the query's stream — every launch of
// the query is ordered behind that stream position anyway (it reads the query) —, so the launches of a query take their
// words without a memset of their own (round 5: 13 hipMemsetAsync per query on a small shard); past the block, or without
// sw_set_query in between, a launch zeroes its own as before.
constexpr uint32_t kWorkZeroBlock = 64;
hipError_t take_work_slot(sw_ctx* ctx, hipStream_t stream, uint32_t** out) {
    uint32_t* w = ctx->d_work + 2 * (ctx->work_next++ % kWorkSlots);
    *out = w;
    if (ctx->work_zeroed > 0) { ctx->work_zeroed--; return hipSuccess; }
    return hipMemsetAsync(w, 0, 2 * sizeof(uint32_t), stream);
}

// The one-shot start / dry signals (sw_set_start_signal, sw_set_dry_signal).  An entry point takes them from the context
// exactly once and hands them down: whatever happens to the call, the pending signals belong to it (an error or an empty
// launch cancels them: nothing will fire, the caller must not wait).
struct Signals {
    uint32_t* start = nullptr;
    uint32_t* dry = nullptr;
};
Signals take_signals(sw_ctx* ctx) {
    const Signals sg{ctx->start_signal, ctx->dry_signal};
    ctx->start_signal = nullptr;
    ctx->dry_signal = nullptr;
    return sg;
}

// CUDASW4_AMD_CHECK_BOUNDS=1: the max_subject_len contract, verified on the device before a scan or a row-pipeline launch
// (the kernels never compare a subject's length with what the caller declared: columns beyond it would be dropped silently)
int check_max_subject_len(sw_ctx* ctx, const int32_t* lengths, const int32_t* positions, const int32_t* count_ptr, int32_t first_pos,
                          int32_t n, int32_t max_subject_len, hipStream_t stream) {
    if (!ctx->check_bounds) return SW_OK;
    int32_t* slot = reinterpret_cast<int32_t*>(ctx->d_zeros + 64);
    int32_t longest = 0;
    SW_HIP(hipMemsetAsync(slot, 0, sizeof(int32_t), stream));
    hipLaunchKernelGGL(max_length_kernel, dim3(std::min(1024, (n + 255) / 256)), dim3(256), 0, stream, lengths, positions, count_ptr, first_pos, n, slot);
    SW_HIP(hipGetLastError());
    SW_HIP(hipMemcpyAsync(&longest, slot, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    SW_HIP(hipStreamSynchronize(stream));
    if (longest > max_subject_len)
        return fail(SW_ERR_INVALID, "max_subject_len " + std::to_string(max_subject_len) + " under-reports: a subject of the range has " +
                                        std::to_string(longest) + " residues");
    return SW_OK;
}

// the kinds' encodings of the words the host hands the kernels (sw_dp_kernel.hpp: Arith), by kind
struct KindCode {
    swk::u32 (*encode_gap)(int);
    swk::u32 (*zero_at)(int, int);
    swk::u32 (*pos_word)(int);
};
template <int KIND>
constexpr KindCode kind_code() { return {swk::Arith<KIND>::encode_gap, swk::Arith<KIND>::zero_at, swk::Arith<KIND>::pos_word}; }
const KindCode kKindCode[4] = {kind_code<swk::F16X2>(), kind_code<swk::I16X2>(), kind_code<swk::I32>(), kind_code<swk::F32>()};

// Everything of ScanParams that follows from the plan and the gap scores; the buffers are the caller's to fill in.
swk::ScanParams fill_scan_params(const LaunchPlan& lp, int gop, int gex) {
    const KindCode& code = kKindCode[lp.kind];
    const int a = -gex;
    swk::ScanParams p{};
    p.nstripes = lp.nstripes;
    p.gop = code.encode_gap(gop); p.gex = code.encode_gap(gex);
    if (lp.offs) {
        p.gop = code.encode_gap(gop - gex);   // gop slot: gop + a
        p.gex_mag = a;
        // row classes of the kernel that plan (rows, lanes) selects: lowering words at the class wrap / the last row
        const bool uniform = lp.frame == 2;
        const int P = swk::frame_classes(kind_packed(lp.kind), lp.rows, lp.lanes, lp.multi, uniform);
        p.wrap_class = code.encode_gap(-a * P);
        p.wrap_last = code.encode_gap(-a * ((lp.rows - 1) % P + (uniform ? 0 : 1)));
        p.flag_period = (int32_t)lp.flag_period;
        p.renorm_quads = (int32_t)(lp.period / 4);
        p.renorm_word = code.encode_gap(-(int)((int64_t)a * lp.period));
        if (uniform) {
            p.uniform_frame = 1;
            for (int u = 0; u < swk::kLevelWords; u++) p.levels[u] = code.zero_at(a, std::min<int>(u, (int)lp.period + 16));
        }
    }
    // Streamed subjects (sw_stream_kernel.hpp): packed kinds on 16-lane groups, column-offset recurrence, plain ranges
    if (lp.stream_slots >= 1) {
        p.stream_slots = lp.stream_slots; p.stream_cols = lp.stream_cols; p.stream_room = lp.stream_room; p.level_base = lp.stream_base;
        p.jump = lp.stream_jump; p.jump_limit = lp.stream_jump - 4;
        p.jump_word = code.pos_word(lp.stream_jump);
    }
    if (lp.multi) p.lcap = lp.lcap;
    if (lp.chain > 1) p.chain = lp.chain;
    // start handshake (sw_set_start_signal): the signal fires once `quorum` workgroups are resident — all of a small
    // launch, the first 64 of a larger one (its remaining workgroups are next in its queue when the waiter is released)
    p.start_quorum = (uint32_t)std::min(lp.grid, 64);
    return p;
}

// overflow lists that are re-scored while they are filled (sw_dp_kernel.hpp: ScanParams::claim / service)
struct ListMode {
    int32_t* claim = nullptr;          // the list, writable: entries are taken by compare-and-swap
    int service_workgroups = 0;        // > 0: a service launch of this many workgroups
    const uint32_t* done_flag = nullptr;
    uint32_t done_value = 0;
};

// what the launching entry points ask plan_launch for ...
LaunchRequest launch_request(int kind, int part_id, int32_t n, int32_t max_subject_len, int gop, int gex, bool ovf_list, size_t scratch,
                             const ListMode& list = ListMode()) {
    LaunchRequest req;
    req.kind = kind; req.part_id = part_id; req.n = n; req.max_subject_len = max_subject_len;
    req.gaps_known = true; req.gop = gop; req.gex = gex; req.ovf_list = ovf_list;
    req.claim = list.claim != nullptr; req.service_workgroups = list.service_workgroups;
    req.scratch = scratch;
    return req;
}
// ... and the sizing and reporting ones: gap scores not known yet, unlimited scratch
LaunchRequest sizing_request(int kind, int part_id, int32_t n, int32_t max_subject_len) {
    LaunchRequest req;
    req.kind = kind; req.part_id = part_id; req.n = n; req.max_subject_len = max_subject_len;
    return req;
}

// Validates the arguments, ensures the profile of the plan's (kind, lanes, frame), fills ScanParams from the plan and launches.
int scan_common(sw_ctx* ctx, const LaunchPlan& lp, const Signals& sg, const int8_t* chars, const uint64_t* offsets, const int32_t* lengths,
                const int32_t* positions, const int32_t* count_ptr, int32_t first_pos, int32_t n,
                int32_t max_subject_len, int gop, int gex, float* scores, int32_t* ids, int64_t id_offset,
                int32_t* ovf_pos, int32_t* ovf_count, int ovf_check, void* temp,
                hipStream_t stream, int32_t* stat_count = nullptr, int32_t stat_limit = 0, const ListMode& list = ListMode()) {
    const int kind = lp.kind, lanes = lp.lanes;
    const swk::KindLaunch* kl = kind_launch(kind);
    if (n < 0 || max_subject_len < 0) return fail(SW_ERR_INVALID, "negative count or length");
    if (max_subject_len > SW_MAX_SUBJECT_LEN)
        return fail(SW_ERR_INVALID, "max_subject_len " + std::to_string(max_subject_len) + ": pass the longest subject of the range (lengths[last]), not the partition's nominal boundary");
    if (gop > 0 || gex > 0) return fail(SW_ERR_INVALID, "gap scores must be <= 0");
    if (kind_packed(kind) && (gop < -1000 || gex < -1000)) return fail(SW_ERR_INVALID, "gap score out of range for a 16-bit kind");
    if (!have_scores(ctx)) return fail(SW_ERR_NO_MATRIX, "sw_set_matrix has not been called");
    if (!ctx->plan.have_query) return fail(SW_ERR_NO_QUERY, "sw_set_query has not been called");
    if (n == 0) return SW_OK;
    if (lp.fell_back) { ovf_pos = nullptr; ovf_count = nullptr; ovf_check = 0; }   // (the 32-bit kind flags nothing)
    if (!chars || !offsets || !lengths || !scores || !ids) return fail(SW_ERR_INVALID, "null buffer");
    if (ovf_check && kind_packed(kind) && (!ovf_pos || !ovf_count)) return fail(SW_ERR_INVALID, "overflow check without overflow buffers");
    SW_HIP(hipSetDevice(ctx->device));
    int rc = check_max_subject_len(ctx, lengths, positions, count_ptr, first_pos, n, max_subject_len, stream);
    if (rc != SW_OK) return rc;
    if (kind_packed(kind) && !lp.offs) return fail(SW_ERR_INVALID, "internal: a packed launch without the column-offset recurrence (packed_fallback_kind)");
    rc = ensure_profile(ctx, lp, lp.offs ? -gex : 0, stream);
    if (rc != SW_OK) return rc;

    swk::ScanParams p = fill_scan_params(lp, gop, gex);
    p.claim = list.claim;
    p.service = list.service_workgroups > 0 ? 1 : 0;
    p.done_flag = list.done_flag;
    p.done_value = list.done_value;
    p.chars = chars; p.offsets = offsets; p.lengths = lengths;
    p.positions = positions; p.count_ptr = count_ptr;
    p.first_pos = first_pos; p.n = n;
    p.len_bound = (max_subject_len + 3) & ~3;   // multi-stripe kernels cut a longer subject here, at a whole letter word
    p.profile = ctx->profiles[kind][shape_index(lanes)][lp.frame].dev;
    p.scores = scores; p.ids = ids; p.id_offset = id_offset;
    p.ovf_pos = ovf_pos; p.ovf_count = ovf_count; p.ovf_check = (ovf_check && kind_packed(kind)) ? 1 : 0;
    p.zeros = ctx->d_zeros + kind * 16;
    p.stat_count = stat_count; p.stat_limit = stat_limit;
    if (lp.chain > 1) p.chain_all = ctx->plan.chain_all ? 1 : 0;
    if (lp.multi) {
        // (sw_scan_temp_bytes asks for the context's setting; a smaller scratch shortens the rounds and the chains, down to
        // one batch per claim, and then the grid: plan_launch)
        if (lp.scratch_too_small) return fail(SW_ERR_TEMP, "temp buffer too small for a multi-stripe query");
        p.scratch = static_cast<uint32_t*>(temp);
    }
    // batches are handed out through an atomic counter (longest subjects first): workgroups that start late
    // because another launch still holds the CUs simply take fewer batches
    SW_HIP(take_work_slot(ctx, stream, &p.work_counter));
    p.start_signal = sg.start;
    p.dry_signal = sg.dry;
    // (streamed rounds: the subjects listed for their predecessor's score only are counted apart, sw_set_dirty_counter)
    if (!stat_count && !positions && p.stream_slots > 1 && lanes == 16 && kind_packed(kind)) { p.stat_count = ctx->dirty_counter; p.stat_limit = INT32_MAX; }
    p.dry_value = ctx->dry_value;
    // (the launcher caps the grid at the kernel's resident workgroups minus the reserve and the quorum with it)
    const int reserve = (list.service_workgroups > 0 || list.claim) ? 0 : ctx->grid_reserve;
    SW_HIP(kl->scan(lp.rows, lanes, lp.multi, lp.offs, lp.grid, reserve, stream, p));
    return SW_OK;
}

}  // namespace


namespace swi {
int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
int32_t query_length(const sw_ctx* ctx) { return ctx && ctx->plan.have_query ? ctx->plan.qlen : 0; }
int device_of(const sw_ctx* ctx) { return ctx ? ctx->device : -1; }
int num_cus(const sw_ctx* ctx) { return ctx ? ctx->plan.num_cus : 0; }
const int8_t* matrix(const sw_ctx* ctx, int* dim) {
    if (!ctx || !ctx->have_matrix) return nullptr;
    *dim = ctx->dim;
    return ctx->d_matrix;
}
}  // namespace swi

namespace {
// What sw_set_query and sw_set_query_pssm share: `bytes` of query data, written by `fill` into a pinned staging buffer,
// uploaded stream-ordered into *dev (grown on demand), and the book-keeping of a new query.
template <class Fill>
int install_query(sw_ctx* ctx, int8_t** dev, size_t* dev_capacity, size_t bytes, int32_t qlen, bool pssm, void* stream, Fill fill) {
    SW_HIP(hipSetDevice(ctx->device));
    if (bytes > *dev_capacity) {
        if (*dev) SW_HIP(hipFree(*dev));
        *dev = nullptr;
        *dev_capacity = 0;
        const size_t cap = std::max<size_t>((bytes + 4095) / 4096 * 4096 * 2, size_t(1) << 16);
        SW_HIP(hipMalloc(dev, cap));
        *dev_capacity = cap;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    // Pinned staging ring: the caller's buffer is copied on the host (a few KB) and is free again on return; the upload
    // itself is stream-ordered — behind the scans of the previous query that still read d_query or its profiles on `s`
    // — and nothing here waits for the GPU unless the ring has wrapped around onto a copy that is still in flight.
    const int slot = ctx->query_next;
    ctx->query_next = (ctx->query_next + 1) % sw_ctx::kQuerySlots;
    if (ctx->query_slot_used[slot]) SW_HIP(hipEventSynchronize(ctx->query_copied[slot]));
    if (bytes > ctx->h_query_capacity[slot]) {
        if (ctx->h_query[slot]) SW_HIP(hipHostFree(ctx->h_query[slot]));
        ctx->h_query[slot] = nullptr;
        ctx->h_query_capacity[slot] = 0;
        const size_t cap = std::max<size_t>((bytes + 4095) / 4096 * 4096 * 2, size_t(1) << 16);
        SW_HIP(hipHostMalloc(&ctx->h_query[slot], cap));
        ctx->h_query_capacity[slot] = cap;
    }
    if (!ctx->query_copied[slot]) SW_HIP(hipEventCreateWithFlags(&ctx->query_copied[slot], hipEventDisableTiming));
    fill(ctx->h_query[slot]);
    SW_HIP(hipMemcpyAsync(*dev, ctx->h_query[slot], bytes, hipMemcpyHostToDevice, s));
    // the control words of this query's launches, zeroed in one go (take_work_slot)
    ctx->work_next = (ctx->work_next + kWorkZeroBlock - 1) / kWorkZeroBlock * kWorkZeroBlock;
    SW_HIP(hipMemsetAsync(ctx->d_work + 2 * (ctx->work_next % kWorkSlots), 0, 2 * kWorkZeroBlock * sizeof(uint32_t), s));
    ctx->work_zeroed = kWorkZeroBlock;
    SW_HIP(hipEventRecord(ctx->query_copied[slot], s));
    ctx->query_slot_used[slot] = true;
    ctx->plan.qlen = qlen;
    ctx->plan.have_query = true;
    ctx->pssm_mode = pssm;
    refresh_score_max(ctx);
    // every switch of query — letters or PSSM, either way round — leaves the cached profiles stale
    for (auto& row : ctx->profiles)
        for (auto& shape : row)
            for (auto& pr : shape) pr.valid = false;
    return SW_OK;
}
}  // namespace

extern "C" {

const char* sw_version(void) { return "cudasw4_amd 0.2 (gfx950)"; }

const char* sw_last_error(void) { return g_last_error.c_str(); }

int sw_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int sw_ctx_create(int device, sw_ctx** out) {
    if (!out) return fail(SW_ERR_INVALID, "null out pointer");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(SW_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= n) return fail(SW_ERR_INVALID, "device index out of range");
    SW_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    SW_HIP(hipGetDeviceProperties(&prop, device));
    sw_ctx* ctx = new sw_ctx;
    ctx->device = device;
    ctx->plan.num_cus = prop.multiProcessorCount;
    swp::settings_from_env(ctx->plan);
    if (const char* e = getenv("CUDASW4_AMD_CHECK_BOUNDS")) ctx->check_bounds = e[0] == '1';
    if (const char* e = getenv("CUDASW4_AMD_PIPE_SPIN_LIMIT")) ctx->pipe_spin_limit = (uint32_t)std::max(1ll, atoll(e));
    if (const char* e = getenv("CUDASW4_AMD_PIPE_TEST_DROP_STAGE")) ctx->pipe_drop_stage = atoi(e);
    if (const char* e = getenv("CUDASW4_AMD_PIPE_CPL")) ctx->pipe_cpl = atoi(e);
    hipError_t e = hipMalloc(&ctx->d_matrix, 26 * swk::kLetters);
    if (e == hipSuccess) e = hipMalloc(&ctx->d_zeros, 256 + 64);  // + the word of the CUDASW4_AMD_CHECK_BOUNDS check (word 64) and the two of sw_streams_run_concurrently (72, 73)
    if (e == hipSuccess) e = hipMalloc(&ctx->d_work, 2 * kWorkSlots * sizeof(uint32_t));
    if (e == hipSuccess) {
        uint32_t z[64] = {};
        for (int i = 0; i < 16; i++) z[SW_KIND_I16X2 * 16 + i] = swk::Arith<swk::I16X2>::kZero;
        e = hipMemcpy(ctx->d_zeros, z, sizeof(z), hipMemcpyHostToDevice);
    }
    // load the four kinds' code objects now (an empty launch each) rather than inside the first query's scan
    for (int kind = 0; kind < 4 && e == hipSuccess; kind++) e = kind_launch(kind)->warm(nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { delete ctx; return fail(SW_ERR_HIP, std::string("context set-up: ") + hipGetErrorString(e)); }
    *out = ctx;
    return SW_OK;
}

int sw_ctx_destroy(sw_ctx* ctx) {
    if (!ctx) return SW_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->d_matrix) (void)hipFree(ctx->d_matrix);
    if (ctx->d_zeros) (void)hipFree(ctx->d_zeros);
    if (ctx->d_work) (void)hipFree(ctx->d_work);
    if (ctx->d_query) (void)hipFree(ctx->d_query);
    if (ctx->d_pssm) (void)hipFree(ctx->d_pssm);
    for (int i = 0; i < sw_ctx::kQuerySlots; i++) {
        if (ctx->h_query[i]) (void)hipHostFree(ctx->h_query[i]);
        if (ctx->query_copied[i]) (void)hipEventDestroy(ctx->query_copied[i]);
    }
    for (auto& row : ctx->profiles)
        for (auto& shape : row)
            for (auto& pr : shape) {
                if (pr.dev) (void)hipFree(pr.dev);
                if (pr.ready) (void)hipEventDestroy(pr.ready);
            }
    delete ctx;
    return SW_OK;
}

int sw_set_matrix(sw_ctx* ctx, const int8_t* matrix_host, int dim) {
    if (!ctx || !matrix_host) return fail(SW_ERR_INVALID, "null argument");
    if (dim != 21 && dim != 25) return fail(SW_ERR_INVALID, "substitution matrices are 21 x 21 (20 amino acids + other) or 25 x 25 (types.hpp:205-396)");
    // internal form: one row per query letter (dim of them) + the row of the query's padding, 21 columns = the dbdata
    // alphabet of the subjects (codes 0..19, 20 = "other" and padding).  25-letter tables: subject code 20 is scored with
    // the table's X column (index 23), the padding row is the X row; both must be negative so that padding neutralises itself.
    constexpr int kX = 23;
    int8_t m[26 * swk::kLetters];
    auto subject_col = [&](int j) { return (dim == 25 && j == swk::kPadLetter) ? kX : j; };
    for (int i = 0; i <= dim; i++) {
        const int qi = i < dim ? i : (dim == 25 ? kX : swk::kPadLetter);
        for (int j = 0; j < swk::kLetters; j++) m[i * swk::kLetters + j] = matrix_host[qi * dim + subject_col(j)];
    }
    for (int i = 0; i <= dim; i++)
        if (m[i * swk::kLetters + swk::kPadLetter] >= 0) return fail(SW_ERR_INVALID, "scores against the padding letter must be negative");
    for (int j = 0; j < swk::kLetters; j++)
        if (m[dim * swk::kLetters + j] >= 0) return fail(SW_ERR_INVALID, "scores against the padding letter must be negative");
    SW_HIP(hipSetDevice(ctx->device));
    SW_HIP(hipMemcpy(ctx->d_matrix, m, (size_t)(dim + 1) * swk::kLetters, hipMemcpyHostToDevice));
    ctx->matrix_max = 1;
    for (int i = 0; i < dim * dim; i++) ctx->matrix_max = std::max(ctx->matrix_max, (int)matrix_host[i]);
    refresh_score_max(ctx);
    if (ctx->plan.have_query && !ctx->pssm_mode && dim < ctx->dim) ctx->plan.have_query = false;  // the installed query may hold codes of the larger alphabet
    ctx->dim = dim;
    ctx->have_matrix = true;
    for (auto& row : ctx->profiles)
        for (auto& shape : row)
            for (auto& pr : shape) pr.valid = false;
    return SW_OK;
}

int sw_set_query(sw_ctx* ctx, const int8_t* query_codes_host, int32_t qlen, void* stream) {
    if (!ctx || !query_codes_host) return fail(SW_ERR_INVALID, "null argument");
    if (qlen <= 0) return fail(SW_ERR_INVALID, "query length must be positive");
    for (int32_t i = 0; i < qlen; i++)
        if (query_codes_host[i] < 0 || query_codes_host[i] >= ctx->dim) return fail(SW_ERR_INVALID, "query code out of range for the installed matrix");
    return install_query(ctx, &ctx->d_query, &ctx->query_capacity, (size_t)qlen, qlen, false, stream,
                         [&](int8_t* staged) { memcpy(staged, query_codes_host, (size_t)qlen); });
}

int sw_set_query_pssm(sw_ctx* ctx, const int8_t* pssm_host, int32_t qlen, void* stream) {
    if (!ctx || !pssm_host) return fail(SW_ERR_INVALID, "null argument");
    if (qlen <= 0) return fail(SW_ERR_INVALID, "query length must be positive");
    if (qlen > SW_PSSM_MAX_QUERY_LEN) return fail(SW_ERR_INVALID, "PSSM query longer than SW_PSSM_MAX_QUERY_LEN");
    int top = 1;
    for (int32_t i = 0; i < qlen; i++) {
        const int8_t* row = pssm_host + (size_t)i * swk::kLetters;
        if (row[swk::kPadLetter] >= 0)
            return fail(SW_ERR_INVALID, "PSSM row " + std::to_string(i) + ": the score against the padding letter (column 20) must be negative");
        for (int j = 0; j < swk::kLetters; j++) top = std::max(top, (int)row[j]);
    }
    const int64_t rows = swk::pssm_staged_rows(qlen);
    const int rc = install_query(ctx, &ctx->d_pssm, &ctx->pssm_capacity, (size_t)rows * swk::kPssmTileLetters, qlen, true, stream, [&](int8_t* staged) {
        memset(staged, (unsigned char)(int8_t)swk::kPssmPadScore, (size_t)rows * swk::kPssmTileLetters);
        for (int32_t i = 0; i < qlen; i++)
            for (int j = 0; j < swk::kLetters; j++) staged[swk::pssm_index(i, j)] = pssm_host[(size_t)i * swk::kLetters + j];
    });
    if (rc == SW_OK) { ctx->pssm_max = top; refresh_score_max(ctx); }
    return rc;
}

int sw_query_is_pssm(const sw_ctx* ctx) { return ctx && ctx->plan.have_query && ctx->pssm_mode ? 1 : 0; }

namespace {
__global__ void __launch_bounds__(256) check_codes_kernel(const int8_t* __restrict__ chars, size_t n, int32_t* bad) {
    const size_t stride = (size_t)gridDim.x * blockDim.x * 16;
    unsigned m = 0;
    // 16 bytes per lane where the pointer allows, the ragged ends byte by byte
    const size_t head = (16 - ((size_t)chars & 15)) & 15;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < head && tid < n) m |= (unsigned char)chars[tid] > 20 ? 1u : 0u;
    const size_t body = n > head ? (n - head) / 16 * 16 : 0;
    for (size_t i = tid * 16; i < body; i += stride) {
        const uint4 v = *reinterpret_cast<const uint4*>(chars + head + i);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            // a byte is > 20 iff it has a bit of 0xE0 set, or it is 21..31: (b + 11) carries into bit 5
            m |= w[k] & 0xE0E0E0E0u;
            m |= ((w[k] & 0x1F1F1F1Fu) + 0x0B0B0B0Bu) & 0x20202020u;
        }
    }
    const size_t tail0 = head + body;
    if (tail0 + tid < n && tid < 16) m |= (unsigned char)chars[tail0 + tid] > 20 ? 1u : 0u;
    if (m) atomicOr(bad, 1);
}
}  // namespace

int sw_check_letter_codes(sw_ctx* ctx, const int8_t* chars, size_t n, int32_t* bad_flag, void* stream) {
    if (!ctx || !bad_flag) return fail(SW_ERR_INVALID, "null argument");
    if (n == 0) return SW_OK;
    if (!chars) return fail(SW_ERR_INVALID, "null buffer");
    SW_HIP(hipSetDevice(ctx->device));
    const size_t want = (n / 16 + 255) / 256 + 1;
    const int grid = (int)std::min<size_t>(want, (size_t)std::max(1, ctx->plan.num_cus) * 16);
    hipLaunchKernelGGL(check_codes_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), chars, n, bad_flag);
    SW_HIP(hipGetLastError());
    return SW_OK;
}

int sw_set_start_signal(sw_ctx* ctx, uint32_t* signal) {
    if (!ctx) return fail(SW_ERR_INVALID, "null context");
    ctx->start_signal = signal;
    return SW_OK;
}


namespace {
// what both row-parallel entry points check before they touch the device
int rows_common_checks(sw_ctx* ctx, const int8_t* chars, const uint64_t* offsets, const int32_t* lengths, int32_t first_pos, int32_t n,
                       int32_t max_subject_len, int gop, int gex, float* scores, int32_t* ids, bool dry_armed, hipStream_t stream,
                       const char* who) {
    if (dry_armed) return fail(SW_ERR_INVALID, std::string(who) + " never runs dry: sw_set_dry_signal applies to sw_scan_partition launches (the armed signal was cancelled)");
    if (n < 0 || max_subject_len < 0) return fail(SW_ERR_INVALID, "negative count or length");
    if (gop > 0 || gex > 0) return fail(SW_ERR_INVALID, "gap scores must be <= 0");
    if (gop > gex) return fail(SW_ERR_INVALID, std::string(who) + " needs gop <= gex (the prefix form of the horizontal gap)");
    if (gex < -10000 || gop < -100000) return fail(SW_ERR_INVALID, std::string("gap score out of range for ") + who);
    if (!have_scores(ctx)) return fail(SW_ERR_NO_MATRIX, "sw_set_matrix has not been called");
    if (!ctx->plan.have_query) return fail(SW_ERR_NO_QUERY, "sw_set_query has not been called");
    if (n == 0) return SW_OK;
    if (!chars || !offsets || !lengths || !scores || !ids) return fail(SW_ERR_INVALID, "null buffer");
    SW_HIP(hipSetDevice(ctx->device));
    return check_max_subject_len(ctx, lengths, nullptr, nullptr, first_pos, n, max_subject_len, stream);
}

// Columns per lane of a pipeline stage.  Narrow spans finish a row sooner, wide ones keep the number of stages — and of
// hand-offs the first row passes through before the last stage starts — down.  Measured on MI355X (tools/giants_bench.py,
// profiles/r05_giants_bench.txt): a row takes 0.27 / 0.38 / 0.57 us at 4 / 8 / 16 columns per lane, a hand-off 3.6 / 5.0 / 8 us
// (the consumer starts a batch of rows when the producer has finished it), so the launch takes about
// qlen * row + stages * hand-off: the width that minimises that for the current query and the longest subject.
int pipeline_cpl(const sw_ctx* ctx, int32_t n, int32_t max_subject_len) {
    if (ctx->pipe_cpl == 4 || ctx->pipe_cpl == 8 || ctx->pipe_cpl == 16) return ctx->pipe_cpl;
    // (sw_rows_pipeline.hpp: batches of 8 rows for queries up to kPipeShortBatchMaxQuery, of 16 above)
    static const double kRowUs16[3] = {0.27, 0.38, 0.57}, kHopUs16[3] = {3.6, 5.0, 8.0}, kRowUs8[3] = {0.32, 0.42, 0.61}, kHopUs8[3] = {2.4, 3.4, 5.3};
    const bool shortBatch = ctx->plan.qlen <= swk::kPipeShortBatchMaxQuery || ctx->pssm_mode;   // (PSSM stages: always batches of 8)
    const double* kRowUs = shortBatch ? kRowUs8 : kRowUs16;
    const double* kHopUs = shortBatch ? kHopUs8 : kHopUs16;
    int best = 16;
    double bestT = 1e300;
    for (int k = 0; k < 3; k++) {
        const int cpl = 4 << k;
        const double stages = std::max(1.0, std::ceil((double)max_subject_len / (64.0 * cpl)));
        // every stage displaces a wave of the launch it runs beside for as long as it lives, and narrow spans spend more
        // instructions per cell: many subjects at once take wide spans (at most ~3 stages per 4 SIMDs of an MI355X)
        if (cpl < 16 && (double)std::max(n, 1) * stages > 768.0) continue;
        const double t = (double)std::max(ctx->plan.qlen, 1) * kRowUs[k] + stages * kHopUs[k];
        if (t < bestT) { bestT = t; best = cpl; }
    }
    return best;
}
constexpr size_t kPipeCtrlBytes = 16;   // control words of a pipelined launch, in front of its hand-off words
int64_t pipeline_stages(int cpl, int32_t max_subject_len) { return std::max<int64_t>(1, ((int64_t)max_subject_len + 64 * cpl - 1) / (64 * cpl)); }
}  // namespace


size_t sw_scan_rows_pipelined_temp_bytes(sw_ctx* ctx, int32_t n, int32_t max_subject_len) {
    if (!ctx || !ctx->plan.have_query || n <= 0 || max_subject_len < 0) return 0;
    const int64_t tickets = (int64_t)n * pipeline_stages(pipeline_cpl(ctx, n, max_subject_len), max_subject_len);
    return kPipeCtrlBytes + (size_t)tickets * ((size_t)ctx->plan.qlen + 1) * sizeof(unsigned long long);
}

namespace {
// the launch both pipelined entry points share: `tickets` workgroups of one wave, hand-off words at `xfer`
int launch_pipeline(sw_ctx* ctx, swk::PipelineParams& p, int cpl, int64_t stages, int64_t tickets, uint32_t* start_signal, void* xfer,
                    hipStream_t stream) {
    const size_t need = kPipeCtrlBytes + (size_t)tickets * ((size_t)ctx->plan.qlen + 1) * sizeof(unsigned long long);
    const bool pssm = ctx->pssm_mode;
    p.query = pssm ? nullptr : ctx->d_query; p.qlen = ctx->plan.qlen; p.matrix = pssm ? ctx->d_pssm : ctx->d_matrix; p.dim = pssm ? 0 : ctx->dim;
    // the launch's control words sit in front of its hand-off words, in the caller's buffer: one memset for both, and no
    // shared ring that a launch in flight on another stream could still be using
    p.ctrl = static_cast<uint32_t*>(xfer);
    p.xfer = reinterpret_cast<unsigned long long*>(static_cast<char*>(xfer) + kPipeCtrlBytes);
    p.start_signal = start_signal;
    // every workgroup counts itself in, also those whose stage does not exist; the handshake fires once as many are
    // resident as the device holds of them beside a bulk grid that is about to take every other slot — one-wave workgroups
    // at the slot's register size, up to 16 per CU — or all of them, whichever is less (with more tickets than
    // resident slots the bulk launch was released only when almost the whole pipeline had run)
    const int slot_regs = ctx->pipe_slot > 0 ? ctx->pipe_slot : 128;
    const int64_t resident = (int64_t)std::max(1, ctx->plan.num_cus) * 4 * std::max(1, std::min(8, 512 / slot_regs)) / 2;
    p.start_quorum = (uint32_t)std::max<int64_t>(1, std::min(tickets, ctx->pipe_quorum > 0 ? (int64_t)ctx->pipe_quorum : resident));
    p.max_stages = (int32_t)stages;
    p.spin_limit = ctx->pipe_spin_limit;
    p.test_drop_stage = ctx->pipe_drop_stage;
    SW_HIP(hipMemsetAsync(xfer, 0xFF, need, stream));   // "not written yet" / "minus one"
    const dim3 grid((unsigned)tickets), block(64);
    const int slot = ctx->pipe_slot;
#define SW_PIPE_LAUNCH_BP(CPL, B, PSSM)                                                                                          \
    do {                                                                                                                          \
        if (slot == 128) hipLaunchKernelGGL((swk::sw_rows_pipeline_kernel<CPL, 128, B, PSSM>), grid, block, 0, stream, p);        \
        else if (slot == 168) hipLaunchKernelGGL((swk::sw_rows_pipeline_kernel<CPL, 168, B, PSSM>), grid, block, 0, stream, p);   \
        else if (slot == 256) hipLaunchKernelGGL((swk::sw_rows_pipeline_kernel<CPL, 256, B, PSSM>), grid, block, 0, stream, p);   \
        else hipLaunchKernelGGL((swk::sw_rows_pipeline_kernel<CPL, 0, B, PSSM>), grid, block, 0, stream, p);                      \
    } while (0)
#define SW_PIPE_LAUNCH(CPL)                                                                                              \
    do {                                                                                                                 \
        if (pssm) SW_PIPE_LAUNCH_BP(CPL, 8, true);                                                                       \
        else if (ctx->plan.qlen <= swk::kPipeShortBatchMaxQuery) SW_PIPE_LAUNCH_BP(CPL, 8, false);                            \
        else SW_PIPE_LAUNCH_BP(CPL, 16, false);                                                                          \
    } while (0)
    if (cpl == 4) SW_PIPE_LAUNCH(4);
    else if (cpl == 8) SW_PIPE_LAUNCH(8);
    else SW_PIPE_LAUNCH(16);
#undef SW_PIPE_LAUNCH_BP
#undef SW_PIPE_LAUNCH
    SW_HIP(hipGetLastError());
    return SW_OK;
}

// Re-score lists: the entries whose subject is at least min_len residues long (at most `cap` of them) move to a list of
// their own, which the pipelined launch takes; in the original list they are marked taken (compare-and-swap: a re-score
// service may still be claiming entries), so that the ordinary re-score launch behind — in claim mode — skips them.
__global__ void __launch_bounds__(256) pipeline_pick_kernel(int32_t* list, const int32_t* count_ptr, int32_t max_count, const int32_t* lengths,
                                                            int32_t min_len, int32_t cap, int32_t* out_pos, int32_t* out_count) {
    __shared__ int k;
    if (threadIdx.x == 0) k = 0;
    __syncthreads();
    const int32_t cnt = min(*count_ptr, max_count);
    for (int32_t i = threadIdx.x; i < cnt; i += blockDim.x) {
        const int32_t v = __hip_atomic_load(list + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v < 0 || lengths[v] < min_len) continue;
        const int slot = atomicAdd(&k, 1);
        if (slot >= cap) continue;   // (the counter overshoots; what does not fit stays with the ordinary launch)
        if (atomicCAS(list + i, v, swk::kListTaken) == v) out_pos[slot] = v;
        else out_pos[slot] = -1;     // somebody else took it in between: an empty slot (the pipelined kernel skips it)
    }
    __syncthreads();
    if (threadIdx.x == 0) *out_count = min(k, cap);
}
constexpr int32_t kPipeRescoreCap = 64;   // entries of one re-score list that can run pipelined
size_t pipe_rescore_header_bytes() { return 256 + (size_t)kPipeRescoreCap * sizeof(int32_t); }
}  // namespace

int sw_scan_rows_pipelined(sw_ctx* ctx, const int8_t* chars, const uint64_t* offsets, const int32_t* lengths, int32_t first_pos,
                           int32_t n, int32_t max_subject_len, int gop, int gex, float* scores, int32_t* ids, int64_t id_offset,
                           int32_t* fail_count, int32_t* over_limit_count, int32_t* over_limit_count2, int32_t packed_limit,
                           void* temp, size_t temp_bytes, void* stream_) {
    if (!ctx) return fail(SW_ERR_INVALID, "null context");
    const Signals sg = take_signals(ctx);
    uint32_t* const start_signal = sg.start;
    const bool dry_armed = sg.dry != nullptr;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // the prefix runs in the frame H~ - k * gex: columns * |gex| must stay far inside 32 bits
    if ((int64_t)max_subject_len * (int64_t)(-gex) >= ((int64_t)1 << 28)) return fail(SW_ERR_INVALID, "subject length x gap extension out of range for sw_scan_rows_pipelined");
    const int rc = rows_common_checks(ctx, chars, offsets, lengths, first_pos, n, max_subject_len, gop, gex, scores, ids, dry_armed, stream, "sw_scan_rows_pipelined");
    if (rc != SW_OK || n == 0) return rc;
    const int cpl = pipeline_cpl(ctx, n, max_subject_len);
    const int64_t stages = pipeline_stages(cpl, max_subject_len);
    const int64_t tickets = (int64_t)n * stages;
    if (tickets > (int64_t)1 << 24) return fail(SW_ERR_INVALID, "too many pipeline stages for one sw_scan_rows_pipelined launch");
    const size_t need = kPipeCtrlBytes + (size_t)tickets * ((size_t)ctx->plan.qlen + 1) * sizeof(unsigned long long);
    if (!temp || temp_bytes < need) return fail(SW_ERR_TEMP, "temp buffer too small for sw_scan_rows_pipelined (sw_scan_rows_pipelined_temp_bytes)");
    swk::PipelineParams p{};
    p.chars = chars; p.offsets = offsets; p.lengths = lengths; p.first_pos = first_pos; p.n = n;
    p.gop = gop; p.gex = gex; p.scores = scores; p.ids = ids; p.id_offset = id_offset;
    p.fail_count = fail_count;
    p.stat_count = over_limit_count; p.stat_count2 = over_limit_count2; p.stat_limit = packed_limit;
    return launch_pipeline(ctx, p, cpl, stages, tickets, start_signal, temp, stream);
}

size_t sw_rescore_overflow_pipelined_temp_bytes(sw_ctx* ctx, int32_t max_subject_len) {
    if (!ctx || !ctx->plan.have_query || max_subject_len < 0) return 0;
    const int64_t tickets = (int64_t)kPipeRescoreCap * pipeline_stages(pipeline_cpl(ctx, kPipeRescoreCap, max_subject_len), max_subject_len);
    return pipe_rescore_header_bytes() + kPipeCtrlBytes + (size_t)tickets * ((size_t)ctx->plan.qlen + 1) * sizeof(unsigned long long);
}

int sw_rescore_overflow_pipelined(sw_ctx* ctx, int32_t* ovf_pos, const int32_t* ovf_count, int32_t max_count, const int8_t* chars,
                                  const uint64_t* offsets, const int32_t* lengths, int32_t max_subject_len, int32_t min_subject_len,
                                  int gop, int gex, float* scores, int32_t* ids, int64_t id_offset, int32_t* fail_count,
                                  int32_t packed_limit, int32_t* true_overflow_count, void* temp, size_t temp_bytes, void* stream_) {
    if (!ctx) return fail(SW_ERR_INVALID, "null context");
    const bool dry_armed = take_signals(ctx).dry != nullptr;   // (these launches run behind the launch that filled their list: no handshake)
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!ovf_pos || !ovf_count) return fail(SW_ERR_INVALID, "null overflow buffers");
    if (max_count <= 0) return SW_OK;
    if ((int64_t)max_subject_len * (int64_t)(-gex) >= ((int64_t)1 << 28)) return fail(SW_ERR_INVALID, "subject length x gap extension out of range for sw_rescore_overflow_pipelined");
    const int rc = rows_common_checks(ctx, chars, offsets, lengths, 0, 1, max_subject_len, gop, gex, scores, ids, dry_armed, stream, "sw_rescore_overflow_pipelined");
    if (rc != SW_OK) return rc;
    const int cpl = pipeline_cpl(ctx, kPipeRescoreCap, max_subject_len);
    const int64_t stages = pipeline_stages(cpl, max_subject_len);
    const int64_t tickets = (int64_t)kPipeRescoreCap * stages;
    const size_t need = sw_rescore_overflow_pipelined_temp_bytes(ctx, max_subject_len);
    if (!temp || temp_bytes < need) return fail(SW_ERR_TEMP, "temp buffer too small for sw_rescore_overflow_pipelined");
    int32_t* out_count = static_cast<int32_t*>(temp);
    int32_t* out_pos = reinterpret_cast<int32_t*>(static_cast<char*>(temp) + 256);
    hipLaunchKernelGGL(pipeline_pick_kernel, dim3(1), dim3(256), 0, stream, ovf_pos, ovf_count, max_count, lengths, std::max(min_subject_len, 1),
                       kPipeRescoreCap, out_pos, out_count);
    SW_HIP(hipGetLastError());
    swk::PipelineParams p{};
    p.chars = chars; p.offsets = offsets; p.lengths = lengths; p.first_pos = 0; p.n = kPipeRescoreCap;
    p.positions = out_pos; p.count_ptr = out_count;
    p.gop = gop; p.gex = gex; p.scores = scores; p.ids = ids; p.id_offset = id_offset;
    p.fail_count = fail_count;
    p.stat_count = true_overflow_count; p.stat_count2 = nullptr; p.stat_limit = packed_limit;
    return launch_pipeline(ctx, p, cpl, stages, tickets, nullptr, static_cast<char*>(temp) + pipe_rescore_header_bytes(), stream);
}

int sw_set_dirty_counter(sw_ctx* ctx, int32_t* counter) {
    if (!ctx) return fail(SW_ERR_INVALID, "null context");
    ctx->dirty_counter = counter;
    return SW_OK;
}

int sw_set_dry_signal(sw_ctx* ctx, uint32_t* signal, uint32_t value) {
    if (!ctx) return fail(SW_ERR_INVALID, "null context");
    ctx->dry_signal = signal;
    ctx->dry_value = value;
    return SW_OK;
}

int sw_set_long16_min(sw_ctx* ctx, int32_t subjects) {
    if (!ctx) return fail(SW_ERR_INVALID, "null context");
    ctx->plan.long16_min = subjects < 0 ? ctx->long16_min_default : subjects;
    return SW_OK;
}

int sw_set_grid_reserve(sw_ctx* ctx, int32_t workgroups) {
    if (!ctx) return fail(SW_ERR_INVALID, "null context");
    if (workgroups < 0) return fail(SW_ERR_INVALID, "negative reserve");
    ctx->grid_reserve = workgroups;
    return SW_OK;
}

namespace {
__global__ void reduce_windows_kernel(const float* __restrict__ win_scores, const int32_t* __restrict__ win_first,
                                      const int32_t* __restrict__ real_pos, int32_t n_real, float* __restrict__ scores,
                                      int32_t* __restrict__ ids, int64_t id_offset) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_real) return;
    float m = -1.0f;
    for (int32_t w = win_first[i]; w < win_first[i + 1]; w++) m = fmaxf(m, win_scores[w]);
    const int32_t pos = real_pos[i];
    scores[pos] = m;
    ids[pos] = (int32_t)(id_offset + pos);
}
}  // namespace

int32_t sw_window_overlap(sw_ctx* ctx, int gop, int gex) {
    if (!ctx || !ctx->plan.have_query || !have_scores(ctx)) return -1;
    // every gap column costs at least min(|gop|, |gex|); an alignment with a positive score of a query of Q residues has at
    // most Q aligned columns worth at most max(M) each: fewer than Q * max(M) / cost gap columns, Q * (1 + max(M) / cost)
    // subject columns in all
    const int cost = std::min(-gop, -gex);
    if (cost <= 0) return -1;
    const int64_t span = (int64_t)ctx->plan.qlen + (int64_t)ctx->plan.qlen * ctx->plan.score_max / cost + 1;
    return span > 0x3fffffff ? -1 : (int32_t)span;
}

int sw_reduce_windows(sw_ctx* ctx, const float* win_scores, const int32_t* win_first, const int32_t* real_pos, int32_t n_real,
                      float* scores, int32_t* ids, int64_t id_offset, void* stream) {
    if (!ctx) return fail(SW_ERR_INVALID, "null context");
    if (n_real <= 0) return SW_OK;
    if (!win_scores || !win_first || !real_pos || !scores || !ids) return fail(SW_ERR_INVALID, "null buffer");
    SW_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(reduce_windows_kernel, dim3((n_real + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), win_scores,
                       win_first, real_pos, n_real, scores, ids, id_offset);
    SW_HIP(hipGetLastError());
    return SW_OK;
}

int sw_plan_query(int kind, int32_t qlen, int32_t* rows_per_lane, int32_t* nstripes) {
    if (!kind_launch(kind) || qlen <= 0) return fail(SW_ERR_INVALID, "bad kind or query length");
    const QueryPlan pl = plan_query(kind, qlen, 16);
    if (rows_per_lane) *rows_per_lane = pl.rows;
    if (nstripes) *nstripes = pl.nstripes;
    return SW_OK;
}

int sw_plan_launch(sw_ctx* ctx, int kind, int part_id, int32_t n, int32_t max_subject_len, int32_t* effective_kind,
                   int32_t* rows_per_lane, int32_t* nstripes, int32_t* lanes) {
    if (!ctx || !kind_launch(kind)) return fail(SW_ERR_INVALID, "null context or unknown kind");
    if (!ctx->plan.have_query) return fail(SW_ERR_NO_QUERY, "sw_set_query has not been called");
    if (part_id >= SW_NUM_LENGTH_PARTITIONS || max_subject_len < 0) return fail(SW_ERR_INVALID, "bad partition id or length");
    const LaunchPlan lp = swp::plan_launch(ctx->plan, sizing_request(kind, part_id, n, max_subject_len));
    if (effective_kind) *effective_kind = lp.kind;
    if (rows_per_lane) *rows_per_lane = lp.rows;
    if (nstripes) *nstripes = lp.nstripes;
    if (lanes) *lanes = lp.lanes;
    return SW_OK;
}

int sw_launch_vgpr_slot(sw_ctx* ctx, int kind, int part_id, int32_t n, int32_t max_subject_len) {
    if (!ctx || !kind_launch(kind) || !ctx->plan.have_query || part_id >= SW_NUM_LENGTH_PARTITIONS || max_subject_len < 0) return 0;
    return swp::plan_launch(ctx->plan, sizing_request(kind, part_id, n, max_subject_len)).vgpr_slot;
}

int sw_set_rows_pipeline_slot(sw_ctx* ctx, int vgprs) {
    if (!ctx) return fail(SW_ERR_INVALID, "null context");
    if (vgprs != 0 && vgprs != 128 && vgprs != 168 && vgprs != 256) return fail(SW_ERR_INVALID, "a register-file slot is 128, 168 or 256 VGPRs (0: as few as the stage needs)");
    ctx->pipe_slot = vgprs;
    return SW_OK;
}

size_t sw_scan_temp_bytes(sw_ctx* ctx, int kind, int part_id, int32_t n, int32_t max_subject_len) {
    if (!ctx || !ctx->plan.have_query || !kind_launch(kind) || max_subject_len < 0 || n <= 0) return 0;
    return swp::plan_launch(ctx->plan, sizing_request(kind, part_id, n, max_subject_len)).scratch_needed;
}

int sw_scan_partition(sw_ctx* ctx, int kind, int part_id, const int8_t* chars, const uint64_t* offsets,
                      const int32_t* lengths, int32_t first_pos, int32_t n, int32_t max_subject_len, int gop, int gex,
                      float* scores, int32_t* ids, int64_t id_offset, int32_t* ovf_pos, int32_t* ovf_count,
                      int ovf_check, void* temp, size_t temp_bytes, void* stream) {
    if (!ctx) return fail(SW_ERR_INVALID, "null context");
    const Signals sg = take_signals(ctx);
    if (part_id < 0 || part_id >= SW_NUM_LENGTH_PARTITIONS || !kind_launch(kind))
        return fail(SW_ERR_INVALID, part_id < 0 || part_id >= SW_NUM_LENGTH_PARTITIONS ? "partition id out of range" : "unknown kind");
    const LaunchPlan lp = swp::plan_launch(ctx->plan, launch_request(kind, part_id, n, max_subject_len, gop, gex, ovf_check != 0, temp ? temp_bytes : 0));
    return scan_common(ctx, lp, sg, chars, offsets, lengths, nullptr, nullptr, first_pos, n, max_subject_len, gop, gex,
                       scores, ids, id_offset, ovf_pos, ovf_count, ovf_check, temp, static_cast<hipStream_t>(stream));
}

namespace {
// a packed range launch: what sw_packed_launch_falls_back can be asked about
bool packed_range(const sw_ctx* ctx, int kind, int part_id) {
    return ctx && kind_launch(kind) && kind_packed(kind) && ctx->plan.have_query && part_id >= 0 && part_id < SW_NUM_LENGTH_PARTITIONS;
}
__global__ void add_counter_kernel(const int32_t* src, int32_t* dst) {
    if (*src) atomicAdd(dst, *src);
}
}  // namespace

int sw_packed_launch_falls_back(sw_ctx* ctx, int kind, int part_id, int32_t n, int32_t max_subject_len, int gop, int gex) {
    if (!packed_range(ctx, kind, part_id)) return 0;
    return swp::plan_launch(ctx->plan, launch_request(kind, part_id, n, max_subject_len, gop, gex, true, swp::kUnlimitedScratch)).fell_back ? 1 : 0;
}

int sw_scan_partition_counted(sw_ctx* ctx, int kind, int part_id, const int8_t* chars, const uint64_t* offsets,
                              const int32_t* lengths, int32_t first_pos, int32_t n, int32_t max_subject_len, int gop, int gex,
                              float* scores, int32_t* ids, int64_t id_offset, int32_t packed_limit, int32_t* over_limit_count,
                              int32_t* over_limit_total, void* temp, size_t temp_bytes, void* stream) {
    if (!ctx) return fail(SW_ERR_INVALID, "null context");
    const Signals sg = take_signals(ctx);
    LaunchPlan lp;
    if (over_limit_count && packed_range(ctx, kind, part_id))
        lp = swp::plan_launch(ctx->plan, launch_request(kind, part_id, n, max_subject_len, gop, gex, true, temp ? temp_bytes : 0));
    if (!lp.fell_back)
        return fail(SW_ERR_INVALID, "sw_scan_partition_counted: not a packed launch that falls back to its 32-bit kind, or no counter");
    const int rc = scan_common(ctx, lp, sg, chars, offsets, lengths, nullptr, nullptr, first_pos, n, max_subject_len, gop, gex,
                               scores, ids, id_offset, nullptr, nullptr, 0, temp, static_cast<hipStream_t>(stream),
                               over_limit_count, packed_limit);
    if (rc != SW_OK || n == 0 || !over_limit_total) return rc;
    hipLaunchKernelGGL(add_counter_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), over_limit_count, over_limit_total);
    SW_HIP(hipGetLastError());
    return SW_OK;
}

namespace {
// What the overflow re-score entry points share: a list of positions with its count on the device, a 32-bit kind.
// `service`: sw_rescore_service, whose list is still being filled (it needs the flag that says when it is complete).
int rescore_list(sw_ctx* ctx, int kind, const int32_t* ovf_pos, const int32_t* ovf_count, int32_t max_count, const int8_t* chars,
                 const uint64_t* offsets, const int32_t* lengths, int32_t max_subject_len, int gop, int gex, float* scores, int32_t* ids,
                 int64_t id_offset, void* temp, size_t temp_bytes, int32_t packed_limit, int32_t* true_overflow_count, const ListMode& list,
                 bool service, void* stream) {
    if (!ctx) return fail(SW_ERR_INVALID, "null context");
    const Signals sg = take_signals(ctx);
    if (kind != SW_KIND_I32 && kind != SW_KIND_F32) return fail(SW_ERR_INVALID, "overflow re-score needs a 32-bit kind");
    if (service && (!ovf_pos || !ovf_count || !list.done_flag)) return fail(SW_ERR_INVALID, "null overflow buffers or flag");
    if (!ovf_pos || !ovf_count) return fail(SW_ERR_INVALID, "null overflow buffers");
    if (max_count <= 0 || (service && list.service_workgroups <= 0)) return SW_OK;
    // grid sized for max_count; the kernel reads the real count on the device (no host round trip,
    // no device-side launch — cf. float_kernels.cuh:1206-1258)
    const LaunchPlan lp = swp::plan_launch(ctx->plan, launch_request(kind, -1, max_count, max_subject_len, gop, gex, false, temp ? temp_bytes : 0, list));
    return scan_common(ctx, lp, sg, chars, offsets, lengths, ovf_pos, ovf_count, 0, max_count, max_subject_len, gop, gex,
                       scores, ids, id_offset, nullptr, nullptr, 0, temp, static_cast<hipStream_t>(stream),
                       true_overflow_count, packed_limit, list);
}
}  // namespace

int sw_rescore_overflow(sw_ctx* ctx, int kind, const int32_t* ovf_pos, const int32_t* ovf_count, int32_t max_count,
                        const int8_t* chars, const uint64_t* offsets, const int32_t* lengths, int32_t max_subject_len,
                        int gop, int gex, float* scores, int32_t* ids, int64_t id_offset, void* temp,
                        size_t temp_bytes, void* stream) {
    return sw_rescore_overflow_stat(ctx, kind, ovf_pos, ovf_count, max_count, chars, offsets, lengths, max_subject_len, gop, gex,
                                    scores, ids, id_offset, temp, temp_bytes, 0, nullptr, stream);
}

int sw_rescore_overflow_stat(sw_ctx* ctx, int kind, const int32_t* ovf_pos, const int32_t* ovf_count, int32_t max_count,
                             const int8_t* chars, const uint64_t* offsets, const int32_t* lengths, int32_t max_subject_len,
                             int gop, int gex, float* scores, int32_t* ids, int64_t id_offset, void* temp,
                             size_t temp_bytes, int32_t packed_limit, int32_t* true_overflow_count, void* stream) {
    return rescore_list(ctx, kind, ovf_pos, ovf_count, max_count, chars, offsets, lengths, max_subject_len, gop, gex, scores, ids, id_offset,
                        temp, temp_bytes, packed_limit, true_overflow_count, ListMode(), false, stream);
}

size_t sw_rescore_service_temp_bytes(sw_ctx* ctx, int kind, int32_t max_subject_len, int workgroups) {
    if (!ctx || !ctx->plan.have_query || !kind_launch(kind) || max_subject_len < 0 || workgroups <= 0) return 0;
    LaunchRequest req = sizing_request(kind, -1, 0, max_subject_len);
    req.service_workgroups = workgroups;
    return (size_t)workgroups * swp::plan_launch(ctx->plan, req).bytes_per_wg;
}

int sw_rescore_service(sw_ctx* ctx, int kind, int32_t* ovf_pos, const int32_t* ovf_count, int32_t max_count,
                       const int8_t* chars, const uint64_t* offsets, const int32_t* lengths, int32_t max_subject_len,
                       int gop, int gex, float* scores, int32_t* ids, int64_t id_offset, void* temp, size_t temp_bytes,
                       int32_t packed_limit, int32_t* true_overflow_count, const uint32_t* done_flag, uint32_t done_value,
                       int workgroups, void* stream) {
    ListMode lm;
    lm.claim = ovf_pos;
    lm.service_workgroups = workgroups;
    lm.done_flag = done_flag;
    lm.done_value = done_value;
    return rescore_list(ctx, kind, ovf_pos, ovf_count, max_count, chars, offsets, lengths, max_subject_len, gop, gex, scores, ids, id_offset,
                        temp, temp_bytes, packed_limit, true_overflow_count, lm, true, stream);
}

int sw_rescore_overflow_claim(sw_ctx* ctx, int kind, int32_t* ovf_pos, const int32_t* ovf_count, int32_t max_count,
                              const int8_t* chars, const uint64_t* offsets, const int32_t* lengths, int32_t max_subject_len,
                              int gop, int gex, float* scores, int32_t* ids, int64_t id_offset, void* temp, size_t temp_bytes,
                              int32_t packed_limit, int32_t* true_overflow_count, void* stream) {
    ListMode lm;
    lm.claim = ovf_pos;
    return rescore_list(ctx, kind, ovf_pos, ovf_count, max_count, chars, offsets, lengths, max_subject_len, gop, gex, scores, ids, id_offset,
                        temp, temp_bytes, packed_limit, true_overflow_count, lm, false, stream);
}

}  // extern "C"
