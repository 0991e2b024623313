// sw_pssm_build_kernel.hpp — sw_pssm_accumulate (include/cudasw4_amd_pssm.h): residue counts, position-based sequence
// weights and weighted counts of a query's aligned hits.  DESIGN.md "Building a PSSM" has the definition.
//
// Two launches, since a weight needs the finished counts:
//   pssm_count_kernel    counts[i][a] += 1 for every (i, a) a sequence has; `used` += 1 per hit that takes part
//   pssm_weight_kernel   per sequence: w = sum of floor(2^32 / (k_i * counts[i][a])) over its (i, a), reduced over the
//                        wave and stored; then wcounts[i][a] += w over the same (i, a)
//
// Shape: one workgroup = one wave64 per hit; the blocks behind the hits take the master row.  walk_hit is the one walker
// of a hit's CIGAR that both kernels use.  The wave loads 64 run words at a time, and an inclusive wave scan over the
// runs' aligned ('=' / 'X') columns, query advances and subject advances gives every run its first column and its first
// position on both sequences.  Then the lanes take COLUMNS, 64 at a time: a lane finds the run of its column by a binary
// search over the scanned column ends (six ds_bpermute reads, no LDS allocation) and from it its query position and its
// subject letter.  Runs are typically 1-5 columns long, so a lane per run, or a run at a time, would idle most of the
// wave.  'I' and 'D' runs advance the positions and own no column.
//
// Accumulation is integer atomicAdd into global memory (32-bit counts, 64-bit weighted counts): exact and independent of
// order.  Inside one wave the destinations are distinct by construction (a column is one query position), so there is
// nothing to combine before the atomic; what a wave does share, the weight of its sequence, is reduced over the wave and
// written with one plain store.  Positions are checked against qlen and the subject's length before they are used: a
// CIGAR that does not belong to its result adds nothing instead of reaching outside the arrays.  Vector stores only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/cudasw4_amd_pssm.h"

namespace swb {

constexpr int kLanes = 64;
constexpr int kLetters = 20;            // standard residues: the columns of counts / wcounts
constexpr int kMasterSpan = 64 * 64;    // positions of the master row one block of the count kernel takes

struct BuildParams {
    const int8_t* query;
    int32_t qlen, n;
    const int8_t* chars;
    const uint64_t* offsets;
    const int32_t* lengths;
    const sw_align_result* results;
    const uint32_t* cigar;
    const uint8_t* include;
    uint32_t* counts;
    unsigned long long* weights;
    unsigned long long* wcounts;
    int32_t* used;
};

__device__ __forceinline__ bool takes_part(const BuildParams& p, const int32_t h) {
    if (p.include && p.include[h] == 0) return false;
    const sw_align_result& r = p.results[h];
    return r.status == SW_ALIGN_OK && r.cigar_len > 0;
}

// inclusive prefix sum over the wave
__device__ __forceinline__ int32_t wave_scan(int32_t v, const int lane) {
#pragma unroll
    for (int d = 1; d < kLanes; d <<= 1) {
        const int32_t u = __shfl_up(v, d, kLanes);
        if (lane >= d) v += u;
    }
    return v;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = kLanes / 2; d > 0; d >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, d, kLanes);
        const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), d, kLanes);
        v += (unsigned long long)hi << 32 | lo;
    }
    return v;
}

// f(i, a) for every (query position i, subject code a < 20) hit h has, each exactly once, on some lane
template <typename F>
__device__ __forceinline__ void walk_hit(const BuildParams& p, const int32_t h, const int lane, F&& f) {
    const sw_align_result r = p.results[h];
    const uint32_t* words = p.cigar + r.cigar_offset;
    const int8_t* s = p.chars + (p.offsets[h] - p.offsets[0]);
    const int32_t slen = p.lengths[h];
    int32_t q0 = r.q_begin, s0 = r.s_begin;   // positions where the current block of runs starts
    for (int32_t first = 0; first < r.cigar_len; first += kLanes) {
        const uint32_t w = first + lane < r.cigar_len ? words[first + lane] : 0u;
        const int32_t len = (int32_t)(w >> 4);
        const uint32_t op = w & 15u;
        const bool pair = op == SW_CIGAR_EQ || op == SW_CIGAR_X;
        const int32_t cend = wave_scan(pair ? len : 0, lane);                      // aligned columns up to this run's end
        const int32_t qend = wave_scan(pair || op == SW_CIGAR_I ? len : 0, lane);  // query residues ...
        const int32_t send = wave_scan(pair || op == SW_CIGAR_D ? len : 0, lane);  // subject residues ...
        const int32_t qrun = q0 + qend - (pair ? len : 0);   // a pair run's first positions (used for pair runs only)
        const int32_t srun = s0 + send - (pair ? len : 0);
        const int32_t crun = cend - (pair ? len : 0);
        int32_t total = __shfl(cend, kLanes - 1, kLanes);
        if (total > p.qlen) total = p.qlen;   // (more aligned columns than query positions: not a CIGAR of this query)
        for (int32_t c0 = 0; c0 < total; c0 += kLanes) {
            const int32_t c = c0 + lane;
            // the first run whose columns end behind c: the smallest x with cend[x] > c
            int32_t x = 0;
#pragma unroll
            for (int step = kLanes / 2; step > 0; step >>= 1) {
                const int32_t e = __shfl(cend, x + step - 1, kLanes);
                if (e <= c) x += step;
            }
            const int32_t k = c - __shfl(crun, x, kLanes);
            const int32_t i = __shfl(qrun, x, kLanes) + k;
            const int32_t j = __shfl(srun, x, kLanes) + k;
            if (c < total && (uint32_t)i < (uint32_t)p.qlen && (uint32_t)j < (uint32_t)slen) {
                const int32_t a = s[j];
                if (a >= 0 && a < kLetters) f(i, a);
            }
        }
        q0 += __shfl(qend, kLanes - 1, kLanes);
        s0 += __shfl(send, kLanes - 1, kLanes);
    }
}

#ifndef SWB_WALKER_ONLY   // (sw_msa_kernel.hpp takes the parameters, the participation rule and the walker, not the kernels)
// blocks [0, n): the hits; the blocks behind them: kMasterSpan positions of the master row each
__global__ __launch_bounds__(kLanes) void pssm_count_kernel(const BuildParams p) {
    const int lane = threadIdx.x;
    const int32_t b = blockIdx.x;
    if (b < p.n) {
        if (!takes_part(p, b)) return;
        if (lane == 0) atomicAdd(p.used, 1);
        walk_hit(p, b, lane, [&](int32_t i, int32_t a) { atomicAdd(p.counts + (size_t)i * kLetters + a, 1u); });
        return;
    }
    const int64_t begin = (int64_t)(b - p.n) * kMasterSpan;
    for (int64_t i = begin + lane; i < begin + kMasterSpan && i < p.qlen; i += kLanes) {
        const int32_t a = p.query[i];
        if (a >= 0 && a < kLetters) atomicAdd(p.counts + (size_t)i * kLetters + a, 1u);
    }
}

// floor(2^32 / (k_i * counts[i][a])), k_i from the row's 20 counts (80 bytes, 16-byte aligned: five dwordx4 loads)
__device__ __forceinline__ unsigned long long weight_term(const BuildParams& p, const int32_t i, const int32_t a) {
    const uint4* row = reinterpret_cast<const uint4*>(p.counts + (size_t)i * kLetters);
    uint32_t k = 0;
#pragma unroll
    for (int v = 0; v < kLetters / 4; v++) {
        const uint4 c = row[v];
        k += (c.x != 0) + (c.y != 0) + (c.z != 0) + (c.w != 0);
    }
    const unsigned long long c = p.counts[(size_t)i * kLetters + a];   // >= 1: this sequence was counted there
    return c ? (1ull << 32) / (k * c) : 0ull;
}

// blocks [0, n): the hits; block n: the master row (when there is one)
__global__ __launch_bounds__(kLanes) void pssm_weight_kernel(const BuildParams p) {
    const int lane = threadIdx.x;
    const int32_t b = blockIdx.x;
    unsigned long long w = 0;
    if (b < p.n) {
        if (!takes_part(p, b)) return;   // (its weight stays the zero of the memset)
        walk_hit(p, b, lane, [&](int32_t i, int32_t a) { w += weight_term(p, i, a); });
        w = wave_sum(w);
        if (lane == 0) p.weights[b] = w;
        walk_hit(p, b, lane, [&](int32_t i, int32_t a) { atomicAdd(p.wcounts + (size_t)i * kLetters + a, w); });
        return;
    }
    for (int32_t i = lane; i < p.qlen; i += kLanes) {
        const int32_t a = p.query[i];
        if (a >= 0 && a < kLetters) w += weight_term(p, i, a);
    }
    w = wave_sum(w);
    if (lane == 0) p.weights[p.n] = w;
    for (int32_t i = lane; i < p.qlen; i += kLanes) {
        const int32_t a = p.query[i];
        if (a >= 0 && a < kLetters) atomicAdd(p.wcounts + (size_t)i * kLetters + a, w);
    }
}
#endif   // SWB_WALKER_ONLY

}  // namespace swb
