// sw_msa_select_kernel.hpp — sw_msa_select (include/cudasw4_amd_msa_select.h): coverage, identity to the query and the
// diversity selection over the rows of the query-anchored alignment.  DESIGN.md §18 has the definition.
//
// Rows are numbered t here: t = 0 is the master, t = h + 1 is hit h (the order of the selection), padded to 64.
//
//   msa_select_rows_kernel   the rows stage of sw_msa_kernel.hpp (one wave64 per row, every byte decided once, six ballot
//                            planes per 64 positions), copied because that header's kernels belong to sw_msa.hip.  It also
//                            counts pairs(h) (one more ballot) and leaves, per rung, the smallest identity count that makes a
//                            row similar TO this one: thr[k][t] = ceil(P_k * res(t) / 100), "never" for res == 0.
//   msa_levels_kernel<TN>    the hot loop: the bit-sliced compare of the pair stage over the tiles on and below the diagonal.
//                            ident is symmetric, so a tile serves both orders: the level of (g, h) against the lane's own
//                            thresholds (denominator res(h)) and, off the diagonal, the level of (h, g) against row g's
//                            thresholds (denominator res(g)), which are wave-uniform.  A level is the number of rungs at
//                            which the pair is similar: TN integer compares per order, once per pair.  levels[g][h] is one
//                            byte, the row of a kept g contiguous over the rows h it may block.  Column 0 of the tiles gives
//                            ident(master, h).
//   msa_select_kernel        one workgroup of 16 waves; the rungs in order, blocks of 64 rows in order.  `maxlev` (LDS, one
//                            byte per row) is the highest level any kept row has against a row, so "blocked at rung t" is
//                            maxlev > t whatever the rank of the kept row; kept rows are folded into it two at a time, all of
//                            a thread's loads in flight together.  A block is resolved on wave-uniform masks: the
//                            open rows, the rows needed under the thin mask (depth < D), the block's own level bits.  Every
//                            keep adds the row to depth; only when a column reaches D is the needed mask taken again.  depth
//                            and the thin mask live in scratch (qlen may be 2^22).  Every loop has a bound known at launch;
//                            nothing waits on another workgroup.
//   msa_depth_kernel         the depth output from the final states, msa_levels_out_kernel the levels in the caller's order.
//
// Vector stores only, no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/cudasw4_amd_msa_select.h"
#define SWB_WALKER_ONLY   // the kernels of that header belong to sw_pssm_build.hip
#include "sw_pssm_build_kernel.hpp"

namespace sws {

constexpr int kLanes = swb::kLanes;
constexpr int kPlanes = 6;          // code bits 0..4 and "is a residue"
constexpr int kWords = 4;           // words of its rows a wave of the levels kernel holds at a time
constexpr int kTile = 64;
constexpr int kPairWaves = 4;
constexpr int kSelectWaves = 16;
constexpr int kSelectThreads = kSelectWaves * kLanes;
constexpr int kMaxRows = (SW_MSA_SELECT_MAX_HITS + 1 + kTile - 1) / kTile * kTile;
constexpr int32_t kNever = 0x7f7f7f7f;   // a threshold no identity count reaches (and a byte pattern a memset can write)
constexpr int kDepthGroups = 8;
constexpr int kFold = (kMaxRows / 4 + kSelectThreads - 1) / kSelectThreads;   // dwords of maxlev a thread of the select kernel owns

struct SelectParams {
    swb::BuildParams hits;          // query, qlen, n, the hit arrays, include (the output fields are unused)
    int32_t min_coverage, min_query_identity, diff, n_ladder;
    int32_t ladder[SW_MSA_SELECT_MAX_LADDER];
    uint8_t* rows;
    int32_t* residues;
    uint8_t* state;
    int32_t* counts;
    int32_t* depth_out;
    uint8_t* levels_out;
    uint32_t* planes;               // [wpad][kPlanes][rpad]
    int32_t* pairs;                 // [rpad]
    int32_t* mident;                // [rpad]: ident(master, t)
    int32_t* thr;                   // [n_ladder][rpad]
    uint8_t* levels;                // [rpad][rpad]: [g][h] = #{k : similar_{P_k}(g, h)}, 0 on the diagonal
    int32_t* depth;                 // [qlen], the select kernel's own
    uint32_t* thin;                 // [words rounded up to 2]: bit i set iff depth[i] < D
    int32_t words;                  // ceil(qlen / 32)
    int32_t wpad;                   // words rounded up to kWords (the padding is zero)
    int32_t rpad;                   // n + 1 rounded up to 64 (the padding is zero)
};

__device__ __forceinline__ int32_t api_row(const int32_t t, const int32_t n) { return t == 0 ? n : t - 1; }
__device__ __forceinline__ int32_t order_row(const int32_t h, const int32_t n) { return h == n ? 0 : h + 1; }

__device__ __forceinline__ long long wave_scan64(long long v, const int lane) {
#pragma unroll
    for (int d = 1; d < kLanes; d <<= 1) {
        const long long u = __shfl_up(v, d, kLanes);
        if (lane >= d) v += u;
    }
    return v;
}

__device__ __forceinline__ unsigned long long uniform64(const unsigned long long v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (unsigned long long)hi << 32 | lo;
}

typedef unsigned short ushort2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_max_u16(const uint32_t a, const uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(ushort2v, a), __builtin_bit_cast(ushort2v, b)));
}

// 64 positions [chunk, chunk + 64) of row t are final: store the bytes and the two words of every plane
__device__ __forceinline__ void emit_chunk(const SelectParams& p, const int32_t t, const int32_t chunk, const int lane, const uint32_t val,
                                           int32_t& residues, int32_t& pairs) {
    const int32_t qlen = p.hits.qlen;
    const int32_t i = chunk + lane;
    if (p.rows && i < qlen) p.rows[(size_t)api_row(t, p.hits.n) * qlen + i] = (uint8_t)val;
    const bool valid = val < 20u;   // (val is NONE at i >= qlen)
    unsigned long long m[kPlanes];
#pragma unroll
    for (int b = 0; b < 5; b++) m[b] = __ballot(valid && ((val >> b) & 1u));
    m[5] = __ballot(valid);
    residues += __popcll(m[5]);
    pairs += __popcll(__ballot(val <= 20u));
    const int pl = lane >> 1;
    unsigned long long mine = m[0];
#pragma unroll
    for (int b = 1; b < kPlanes; b++) mine = pl == b ? m[b] : mine;
    const int32_t w = chunk / 32 + (lane & 1);
    if (lane < 2 * kPlanes && w < p.words)
        p.planes[((size_t)w * kPlanes + pl) * p.rpad + t] = (lane & 1) ? (uint32_t)(mine >> 32) : (uint32_t)mine;
}

__device__ __forceinline__ void finish_row(const SelectParams& p, const int32_t t, const int lane, const int32_t residues, const int32_t pairs) {
    if (lane == 0) {
        p.residues[api_row(t, p.hits.n)] = residues;
        p.pairs[t] = pairs;
    }
    if (lane < p.n_ladder) p.thr[(size_t)lane * p.rpad + t] = residues > 0 ? (p.ladder[lane] * residues + 99) / 100 : kNever;
}

__global__ __launch_bounds__(kLanes) void msa_select_rows_kernel(const SelectParams p) {
    const int lane = threadIdx.x;
    const int32_t b = blockIdx.x;
    const int32_t qlen = p.hits.qlen, n = p.hits.n;
    int32_t residues = 0, pairs = 0;
    if (b == n) {   // the master
        for (int32_t chunk = 0; chunk < qlen; chunk += kLanes) {
            uint32_t val = SW_MSA_NONE;
            if (p.hits.query && chunk + lane < qlen) {
                const uint32_t a = (uint8_t)p.hits.query[chunk + lane];
                val = a < 20u ? a : 20u;
            }
            emit_chunk(p, 0, chunk, lane, val, residues, pairs);
        }
        finish_row(p, 0, lane, residues, pairs);
        return;
    }
    const int32_t t = b + 1;
    int32_t chunk = 0;              // the first position that is not final yet (a multiple of 64)
    uint32_t val = SW_MSA_NONE;     // this lane's byte of the chunk so far
    const sw_align_result r = p.hits.results[b];
    if (swb::takes_part(p.hits, b) && r.q_begin >= 0 && r.s_begin >= 0) {
        const uint32_t* words = p.hits.cigar + r.cigar_offset;
        const int8_t* s = p.hits.chars + (p.hits.offsets[b] - p.hits.offsets[0]);
        const long long slen = p.hits.lengths[b];
        long long q0 = r.q_begin, s0 = r.s_begin;   // positions where the current block of runs starts
        for (; chunk + kLanes <= q0 && chunk < qlen; chunk += kLanes) emit_chunk(p, t, chunk, lane, SW_MSA_NONE, residues, pairs);
        for (int32_t first = 0; first < r.cigar_len && q0 < qlen; first += kLanes) {
            const uint32_t w = first + lane < r.cigar_len ? words[first + lane] : 0u;
            const long long len = (long long)(w >> 4);
            const uint32_t op = w & 15u;
            const bool pair = op == SW_CIGAR_EQ || op == SW_CIGAR_X;
            const long long qadv = pair || op == SW_CIGAR_I ? len : 0;
            const long long sadv = pair || op == SW_CIGAR_D ? len : 0;
            const long long qend = wave_scan64(qadv, lane);    // query residues up to this run's end, from q0
            const long long send = wave_scan64(sadv, lane);
            const long long qrun = qend - qadv, srun = s0 + send - sadv;   // the run's first positions
            const long long qe = q0 + __shfl(qend, kLanes - 1, kLanes);  // the block of runs covers [q0, qe)
            while (chunk < qlen && chunk < qe) {
                const long long i = (long long)chunk + lane;
                const long long rel = i - q0;
                // the run that covers rel: the smallest x with qend[x] > rel (runs without query residues are skipped);
                // every lane takes the shuffles, the lanes outside the block's positions drop what they found
                int32_t x = 0;
#pragma unroll
                for (int step = kLanes / 2; step > 0; step >>= 1) {
                    const long long e = __shfl(qend, x + step - 1, kLanes);
                    if (e <= rel) x += step;
                }
                const long long k = rel - __shfl(qrun, x, kLanes);
                const long long j = __shfl(srun, x, kLanes) + k;
                const uint32_t xop = __shfl(op, x, kLanes);
                if (i >= q0 && i < qe && i < qlen) {
                    if (xop == SW_CIGAR_I) {
                        val = i < r.q_end ? SW_MSA_GAP : SW_MSA_NONE;
                    } else if (j >= 0 && j < slen) {   // ('=' / 'X': only these and 'I' advance the query)
                        const uint32_t a = (uint8_t)s[j];
                        val = a < 20u ? a : 20u;
                    }
                }
                if ((long long)chunk + kLanes > qe) break;   // the next block of runs has more of this chunk
                emit_chunk(p, t, chunk, lane, val, residues, pairs);
                val = SW_MSA_NONE;
                chunk += kLanes;
            }
            q0 = qe;
            s0 += __shfl(send, kLanes - 1, kLanes);
        }
    }
    for (; chunk < qlen; chunk += kLanes) {
        emit_chunk(p, t, chunk, lane, val, residues, pairs);
        val = SW_MSA_NONE;
    }
    finish_row(p, t, lane, residues, pairs);
}

// grid (ceil(tiles / kPairWaves), tiles): wave w of block x takes the rows h of tile x * kPairWaves + w against the rows g
// of tile blockIdx.y.  TN: the rungs the epilogue compares (n_ladder <= TN; the rungs beyond n_ladder never match).
template <int TN>
__global__ __launch_bounds__(kPairWaves * kLanes) void msa_levels_kernel(const SelectParams p) {
    const int lane = threadIdx.x & (kLanes - 1);
    const int32_t htile = blockIdx.x * kPairWaves + (threadIdx.x >> 6);
    const int32_t gtile = blockIdx.y;
    const int32_t tiles = p.rpad / kTile;
    if (htile >= tiles || gtile > htile) return;
    const int32_t th = htile * kTile + lane;
    const uint32_t* __restrict__ planes = p.planes;
    const size_t rpad = (size_t)p.rpad;
    uint32_t acc[kTile];
#pragma unroll
    for (int g = 0; g < kTile; g++) acc[g] = 0;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for (int32_t w0 = 0; w0 < p.wpad; w0 += kWords) {
        uint32_t hp[kWords][kPlanes];
#pragma unroll
        for (int k = 0; k < kWords; k++)
#pragma unroll
            for (int pl = 0; pl < kPlanes; pl++) hp[k][pl] = planes[((size_t)(w0 + k) * kPlanes + pl) * rpad + th];
        const uint32_t* __restrict__ gbase = planes + (size_t)w0 * kPlanes * rpad + (size_t)gtile * kTile;   // wave-uniform
        // two rows g at a time behind a scheduling barrier (left alone, the scheduler loads the whole tile's
        // scalar words first and spills scalar registers by the thousand)
#pragma unroll
        for (int g = 0; g < kTile; g += 2) {
#pragma unroll
            for (int k = 0; k < kWords; k++) {
#pragma unroll
                for (int d = 0; d < 2; d++) {
                    const uint32_t* gp = gbase + (size_t)k * kPlanes * rpad + g + d;
                    const uint32_t x = ((hp[k][0] ^ gp[0]) | (hp[k][1] ^ gp[rpad])) | ((hp[k][2] ^ gp[2 * rpad]) | (hp[k][3] ^ gp[3 * rpad])) |
                                       (hp[k][4] ^ gp[4 * rpad]);
                    acc[g + d] += __popc((hp[k][5] & gp[5 * rpad]) & ~x);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const int32_t* __restrict__ thr = p.thr;
    uint8_t* __restrict__ levels = p.levels;
    if (gtile == 0) p.mident[th] = (int32_t)acc[0];
    const bool diagonal = gtile == htile;
    // (g, h): row h is judged, the thresholds are the lane's own
    int32_t mine[TN];
#pragma unroll
    for (int k = 0; k < TN; k++) mine[k] = k < p.n_ladder ? thr[(size_t)k * rpad + th] : kNever;
#pragma unroll
    for (int g = 0; g < kTile; g++) {
        uint32_t lev = 0;
#pragma unroll
        for (int k = 0; k < TN; k++) lev += (int32_t)acc[g] >= mine[k] ? 1u : 0u;
        if (diagonal && g == lane) lev = 0;
        levels[((size_t)gtile * kTile + g) * rpad + th] = (uint8_t)lev;
    }
    if (diagonal) return;
    // (h, g): row g is judged, its thresholds are wave-uniform; four rows g at a time for the same reason as above
    uint32_t* out = reinterpret_cast<uint32_t*>(levels + (size_t)th * rpad + (size_t)gtile * kTile);
    const int32_t* __restrict__ gthr = thr + (size_t)gtile * kTile;
#pragma unroll
    for (int g4 = 0; g4 < kTile / 4; g4++) {
        uint32_t packed = 0;
#pragma unroll
        for (int d = 0; d < 4; d++) {
            uint32_t lev = 0;
#pragma unroll
            for (int k = 0; k < TN; k++) {
                const int32_t need = k < p.n_ladder ? gthr[(size_t)k * rpad + g4 * 4 + d] : kNever;
                lev += (int32_t)acc[g4 * 4 + d] >= need ? 1u : 0u;
            }
            packed |= lev << (8 * d);
        }
        out[g4] = packed;
        __builtin_amdgcn_sched_barrier(0);
    }
}

// one workgroup of kSelectWaves waves
__global__ __launch_bounds__(kSelectThreads) void msa_select_kernel(const SelectParams p) {
    __shared__ uint32_t maxlev[kMaxRows / 4];                 // one byte per row t: the highest level of a kept row against it
    __shared__ unsigned long long cand[kMaxRows / kTile];     // the candidates of every block of 64 rows
    __shared__ unsigned long long own[kTile];                 // bit g of own[l]: levels[block row g][block row l] > rung
    __shared__ uint32_t ownpart[kSelectWaves][kTile];
    __shared__ unsigned long long needpart[kSelectWaves];
    const int tid = threadIdx.x;
    const int lane = tid & (kLanes - 1);
    const int wave = tid >> 6;
    const int32_t n = p.hits.n, qlen = p.hits.qlen, rpad = p.rpad, words = p.words;
    const int32_t tiles = rpad / kTile;
    const int32_t D = p.diff, T = p.n_ladder;
    const uint8_t* __restrict__ levels = p.levels;
    const uint32_t* __restrict__ planes = p.planes;
    uint32_t* thin = p.thin;      // (written here: never behind a scalar load)
    int32_t* depth = p.depth;

    // row tk is kept: its residues go into depth, the columns that reach D leave the thin mask.  Column i is always this
    // thread's, a thin word always its wave's.  -> whether the thin mask changed (the same for every thread)
    auto add_depth = [&](const int32_t tk) -> bool {
        int reached = 0;
        for (int32_t base = wave * kLanes; base < qlen; base += kSelectThreads) {
            const int32_t i = base + lane;
            const int32_t w = i >> 5;
            bool r = false;
            if (i < qlen && (planes[((size_t)w * kPlanes + 5) * rpad + tk] >> (i & 31) & 1u)) {
                const int32_t d = depth[i] + 1;
                depth[i] = d;
                r = d == D;
            }
            const unsigned long long m = __ballot(r);
            if (m) {
                if (lane == 0 && (uint32_t)m) thin[w] &= ~(uint32_t)m;
                if (lane == 32 && (uint32_t)(m >> 32)) thin[w] &= ~(uint32_t)(m >> 32);
                reached = 1;
            }
        }
        return __syncthreads_or(reached) != 0;
    };
    // the rows `kept` of block b are kept: their levels against every row go into maxlev
    // Every thread owns the same kFold dwords of maxlev throughout; the rows are taken two at a time with all of a thread's
    // loads issued before the first is used (one load at a time, the latency of 4 000 dependent loads per thread was the
    // whole stage), and the byte-wise maximum is two packed 16-bit ones over the even and the odd bytes.
    auto add_levels = [&](const int32_t b, unsigned long long kept) {
        uint32_t even[kFold], odd[kFold];
#pragma unroll
        for (int j = 0; j < kFold; j++) {
            const int32_t q = tid + j * kSelectThreads;
            const uint32_t m = q < rpad / 4 ? maxlev[q] : 0u;
            even[j] = m & 0x00ff00ffu;
            odd[j] = m >> 8 & 0x00ff00ffu;
        }
        for (int pass = 0; pass < kTile / 2 && kept; pass++) {
            const int k0 = __builtin_ctzll(kept);
            kept &= kept - 1;
            const int k1 = kept ? __builtin_ctzll(kept) : k0;   // (an odd row out is folded twice)
            kept &= kept - 1;
            const uint32_t* r0 = reinterpret_cast<const uint32_t*>(levels + (size_t)(b * kTile + k0) * rpad);
            const uint32_t* r1 = reinterpret_cast<const uint32_t*>(levels + (size_t)(b * kTile + k1) * rpad);
            uint32_t v0[kFold], v1[kFold];
#pragma unroll
            for (int j = 0; j < kFold; j++) {
                const int32_t q = tid + j * kSelectThreads;
                v0[j] = q < rpad / 4 ? r0[q] : 0u;
                v1[j] = q < rpad / 4 ? r1[q] : 0u;
            }
#pragma unroll
            for (int j = 0; j < kFold; j++) {
                even[j] = pk_max_u16(pk_max_u16(even[j], v0[j] & 0x00ff00ffu), v1[j] & 0x00ff00ffu);
                odd[j] = pk_max_u16(pk_max_u16(odd[j], v0[j] >> 8 & 0x00ff00ffu), v1[j] >> 8 & 0x00ff00ffu);
            }
        }
#pragma unroll
        for (int j = 0; j < kFold; j++) {
            const int32_t q = tid + j * kSelectThreads;
            if (q < rpad / 4) maxlev[q] = even[j] | odd[j] << 8;
        }
        __syncthreads();
    };

    for (int32_t q = tid; q < rpad / 4; q += kSelectThreads) maxlev[q] = 0;
    if (D > 0) {
        for (int32_t i = tid; i < qlen; i += kSelectThreads) depth[i] = 0;
        const int32_t thinWords = (words + 1) / 2 * 2;
        for (int32_t w = tid; w < thinWords; w += kSelectThreads)
            thin[w] = w >= words ? 0u : (w == words - 1 && (qlen & 31)) ? (1u << (qlen & 31)) - 1u : ~0u;
    }
    // steps 2 .. 5: every hit's state before the rungs (a candidate starts as THINNED and is overwritten when it is kept)
    for (int32_t b = wave; b < tiles; b += kSelectWaves) {
        const int32_t t = b * kTile + lane;
        bool c = false;
        if (t >= 1 && t <= n) {
            const int32_t res = p.residues[t - 1];
            uint8_t st = SW_MSA_STATE_NONE;
            if (res > 0) {
                if (100ll * p.pairs[t] < (long long)p.min_coverage * qlen) st = SW_MSA_STATE_COVERAGE;
                else if (100ll * p.mident[t] < (long long)p.min_query_identity * res) st = SW_MSA_STATE_QUERY_IDENTITY;
                else {
                    st = SW_MSA_STATE_THINNED;
                    c = true;
                }
            }
            p.state[t - 1] = st;
        }
        const unsigned long long m = __ballot(c);
        if (lane == 0) cand[b] = m;
    }
    const bool master = p.residues[n] > 0;
    if (tid == 0) p.state[n] = master ? SW_MSA_STATE_KEPT : SW_MSA_STATE_NONE;
    __syncthreads();
    if (master) {
        if (D > 0) (void)add_depth(0);
        add_levels(0, 1ull);
    }

    for (int32_t rung = 0; rung < T; rung++) {
        for (int32_t b = 0; b < tiles; b++) {
            unsigned long long cm = uniform64(cand[b]);
            if (!cm) continue;
            const int32_t tl = b * kTile + lane;
            const uint32_t lev = maxlev[tl >> 2] >> ((tl & 3) * 8) & 255u;
            const unsigned long long open = uniform64(cm & ~__ballot(lev > (uint32_t)rung));   // the same in every wave
            if (!open) continue;
            {   // the block's own level bits: wave w has the rows g = 4 w .. 4 w + 3
                uint32_t part = 0;
#pragma unroll
                for (int d = 0; d < 4; d++)
                    part |= (levels[(size_t)(b * kTile + wave * 4 + d) * rpad + tl] > (uint32_t)rung ? 1u : 0u) << d;
                ownpart[wave][lane] = part;
            }
            __syncthreads();
            if (wave == 0) {
                unsigned long long o = 0;
#pragma unroll
                for (int w = 0; w < kSelectWaves; w++) o |= (unsigned long long)ownpart[w][lane] << (4 * w);
                own[lane] = o;
            }
            __syncthreads();
            unsigned long long rem = open, kept = 0;
            bool dirty = D > 0;
            for (int it = 0; it <= kTile && rem; it++) {   // (every pass but the last keeps a row)
                if (dirty) {
                    uint32_t nz = 0;
                    if (rem >> lane & 1ull)
                        for (int32_t w = wave; w < words; w += kSelectWaves) nz |= planes[((size_t)w * kPlanes + 5) * rpad + tl] & thin[w];
                    const unsigned long long m = __ballot(nz != 0);
                    if (lane == 0) needpart[wave] = m;
                    __syncthreads();
                    unsigned long long needed = 0;
#pragma unroll
                    for (int w = 0; w < kSelectWaves; w++) needed |= needpart[w];
                    needed = uniform64(needed);
                    __syncthreads();
                    cm &= ~(rem & ~needed);   // not needed now: never again (depth only grows); the state stays THINNED
                    rem &= needed;
                    dirty = false;
                }
                for (int step = 0; step < kTile && rem; step++) {
                    const int k = __builtin_ctzll(rem);
                    const unsigned long long bit = 1ull << k;
                    rem &= ~bit;
                    if (uniform64(own[k]) & kept) continue;   // similar to a row kept in this block at this rung: still a candidate
                    kept |= bit;
                    cm &= ~bit;
                    if (tid == 0) p.state[b * kTile + k - 1] = SW_MSA_STATE_KEPT;
                    if (D > 0 && add_depth(b * kTile + k)) {
                        dirty = true;
                        break;
                    }
                }
            }
            if (tid == 0) cand[b] = cm;
            if (kept) add_levels(b, kept);
            else __syncthreads();
        }
    }
    __syncthreads();
    if (wave == 0) {
        int32_t c[4] = {0, 0, 0, 0};
        for (int32_t b = 0; b < tiles; b++) {
            const int32_t t = b * kTile + lane;
            const uint32_t st = t >= 1 && t <= n ? p.state[t - 1] : 255u;
#pragma unroll
            for (int s = 0; s < 4; s++) c[s] += __popcll(__ballot(st == uint32_t(s + 1)));
        }
        if (lane < 4) p.counts[lane] = lane == 0 ? c[0] : lane == 1 ? c[1] : lane == 2 ? c[2] : c[3];
    }
}

// grid: one block per 32 columns; kDepthGroups groups of 32 threads share the rows
__global__ __launch_bounds__(kDepthGroups * 32) void msa_depth_kernel(const SelectParams p) {
    __shared__ int32_t part[kDepthGroups][32];
    const int col = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int32_t w = blockIdx.x, n = p.hits.n;
    int32_t sum = 0;
    for (int32_t t = grp; t <= n; t += kDepthGroups)
        if (p.state[api_row(t, n)] == SW_MSA_STATE_KEPT) sum += p.planes[((size_t)w * kPlanes + 5) * p.rpad + t] >> col & 1u;
    part[grp][col] = sum;
    __syncthreads();
    if (grp == 0) {
#pragma unroll
        for (int g = 1; g < kDepthGroups; g++) sum += part[g][col];
        const int32_t i = w * 32 + col;
        if (i < p.hits.qlen) p.depth_out[i] = sum;
    }
}

// grid (ceil((n + 1) / 256), n + 1): levels_out[h][g] in the caller's row order
__global__ __launch_bounds__(256) void msa_levels_out_kernel(const SelectParams p) {
    const int32_t n = p.hits.n;
    const int32_t g = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y;
    if (g > n) return;
    p.levels_out[(size_t)h * (n + 1) + g] = p.levels[(size_t)order_row(g, n) * p.rpad + order_row(h, n)];
}

}  // namespace sws
