// sw_msa_kernel.hpp — sw_msa_filter (include/cudasw4_amd_msa.h): the rows of the query-anchored alignment of a query's
// hits, their pairwise identity and the greedy redundancy filter.  DESIGN.md §17 has the definition.
//
// Three launches:
//   msa_rows_kernel    one wave64 per row (blocks [0, n): the hits, block n: the master).  The CIGAR is walked as walk_hit
//                      (sw_pssm_build_kernel.hpp) walks it — 64 run words at a time, wave scans over the runs' advances, a
//                      binary search per lane — but the lanes take QUERY POSITIONS, 64 aligned ones at a time, and a
//                      position's byte is decided once, from the one run that covers it ('=' / 'X': the subject code, 'I':
//                      GAP, no run: NONE), then stored once.  No byte depends on the order of two stores.  The same pass
//                      emits the compare form: six wave ballots per 64 positions (five code-bit planes and the "is a residue"
//                      plane, code bits zero where the byte is no residue) give two 32-bit words per plane.
//   msa_pairs_kernel   the hot loop.  planes are laid out [word][plane][row] with the rows in greedy order (master first), so
//                      lanes = rows h read consecutive addresses.  A wave holds kWords words x 6 planes of its 64 rows h in
//                      registers and walks a tile of 64 earlier rows g, whose words are wave-uniform (scalar loads, scalar
//                      operands); ident over 32 columns is 5 XOR, 4 OR, one AND of the valid planes, one AND-NOT and one
//                      v_bcnt_u32_b32 that accumulates.  64 accumulators per lane; a workgroup is four waves = 256 rows h
//                      against the same 64 rows g, so the g words come out of the scalar cache three times out of four.
//                      Tiles above the diagonal return at once.  The result is the `similar` bit matrix, one 64-bit word per
//                      (g tile, row h), and — for tests — the identity counts themselves.
//   msa_greedy_kernel  one workgroup.  Blocks of 64 rows in order: first every row of the block against the kept rows of all
//                      earlier blocks (16 waves share the g tiles, the keep bits live in LDS), then wave 0 resolves the block
//                      itself, 64 sequential steps on wave-uniform masks.  keep and purged are written with plain stores.
//
// Every index is checked before it is used: a CIGAR that does not belong to its record leaves NONE instead of reaching
// outside the arrays.  Vector stores only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/cudasw4_amd_msa.h"
#define SWB_WALKER_ONLY   // the kernels of that header belong to sw_pssm_build.hip
#include "sw_pssm_build_kernel.hpp"

namespace swm {

constexpr int kLanes = swb::kLanes;
constexpr int kPlanes = 6;          // code bits 0..4 and "is a residue"
constexpr int kWords = 4;           // words of its rows a wave of the pair kernel holds at a time
constexpr int kTile = 64;           // rows g per tile = bits of a `similar` word
constexpr int kPairWaves = 4;
constexpr int kGreedyWaves = 16;

struct MsaParams {
    swb::BuildParams hits;          // query, qlen, n, the hit arrays, include (the output fields are unused)
    int32_t max_identity;
    uint8_t* rows;
    int32_t* residues;
    uint8_t* keep;
    int32_t* purged;
    uint32_t* pair_ident;
    uint32_t* planes;               // [wpad][kPlanes][rpad], rows in greedy order: 0 = master, h + 1 = hit h
    unsigned long long* similar;    // [rpad / kTile][rpad]: bit g of [gt][t] = similar(row gt * 64 + g, row t), g before t
    int32_t words;                  // ceil(qlen / 32)
    int32_t wpad;                   // words rounded up to kWords (the padding is zero)
    int32_t rpad;                   // n + 1 rounded up to 64 (the padding is zero)
};

// greedy order <-> the caller's row index (the master is row n there)
__device__ __forceinline__ int32_t api_row(const int32_t t, const int32_t n) { return t == 0 ? n : t - 1; }

__device__ __forceinline__ long long wave_scan64(long long v, const int lane) {
#pragma unroll
    for (int d = 1; d < kLanes; d <<= 1) {
        const long long u = __shfl_up(v, d, kLanes);
        if (lane >= d) v += u;
    }
    return v;
}

// 64 positions [chunk, chunk + 64) of row t are final: store the bytes and the two words of every plane
__device__ __forceinline__ void emit_chunk(const MsaParams& p, const int32_t t, const int32_t chunk, const int lane, const uint32_t val,
                                           int32_t& residues) {
    const int32_t qlen = p.hits.qlen;
    const int32_t i = chunk + lane;
    if (p.rows && i < qlen) p.rows[(size_t)api_row(t, p.hits.n) * qlen + i] = (uint8_t)val;
    const bool valid = val < 20u;   // (val is NONE at i >= qlen)
    unsigned long long m[kPlanes];
#pragma unroll
    for (int b = 0; b < 5; b++) m[b] = __ballot(valid && ((val >> b) & 1u));
    m[5] = __ballot(valid);
    residues += __popcll(m[5]);
    const int pl = lane >> 1;
    unsigned long long mine = m[0];
#pragma unroll
    for (int b = 1; b < kPlanes; b++) mine = pl == b ? m[b] : mine;
    const int32_t w = chunk / 32 + (lane & 1);
    if (lane < 2 * kPlanes && w < p.words)
        p.planes[((size_t)w * kPlanes + pl) * p.rpad + t] = (lane & 1) ? (uint32_t)(mine >> 32) : (uint32_t)mine;
}

__global__ __launch_bounds__(kLanes) void msa_rows_kernel(const MsaParams p) {
    const int lane = threadIdx.x;
    const int32_t b = blockIdx.x;
    const int32_t qlen = p.hits.qlen, n = p.hits.n;
    int32_t residues = 0;
    if (b == n) {   // the master
        for (int32_t chunk = 0; chunk < qlen; chunk += kLanes) {
            uint32_t val = SW_MSA_NONE;
            if (p.hits.query && chunk + lane < qlen) {
                const uint32_t a = (uint8_t)p.hits.query[chunk + lane];
                val = a < 20u ? a : 20u;
            }
            emit_chunk(p, 0, chunk, lane, val, residues);
        }
        if (lane == 0) p.residues[n] = residues;
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
        for (; chunk + kLanes <= q0 && chunk < qlen; chunk += kLanes) emit_chunk(p, t, chunk, lane, SW_MSA_NONE, residues);
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
                emit_chunk(p, t, chunk, lane, val, residues);
                val = SW_MSA_NONE;
                chunk += kLanes;
            }
            q0 = qe;
            s0 += __shfl(send, kLanes - 1, kLanes);
        }
    }
    for (; chunk < qlen; chunk += kLanes) {
        emit_chunk(p, t, chunk, lane, val, residues);
        val = SW_MSA_NONE;
    }
    if (lane == 0) p.residues[b] = residues;
}

__device__ __forceinline__ int32_t residues_of(const MsaParams& p, const int32_t t) {
    return t <= p.hits.n ? p.residues[api_row(t, p.hits.n)] : 0;
}

// grid (ceil(tiles / kPairWaves), tiles): wave w of block x takes the rows h of tile x * kPairWaves + w against the rows g
// of tile blockIdx.y
template <bool IDENT>
__global__ __launch_bounds__(kPairWaves * kLanes) void msa_pairs_kernel(const MsaParams p) {
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
        // two rows g at a time (their words are neighbours: 24 two-dword scalar loads), and nothing moves across the pairs:
        // left alone, the scheduler loads the whole tile's 1536 words first and spills scalar registers by the thousand
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
    const int32_t n = p.hits.n;
    const unsigned long long res = (unsigned long long)residues_of(p, th);
    if (p.similar) {
        unsigned long long bits = 0;
#pragma unroll
        for (int g = 0; g < kTile; g++) {
            const bool sim = gtile * kTile + g < th && res > 0 && 100ull * acc[g] >= (unsigned long long)p.max_identity * res;
            bits |= sim ? 1ull << g : 0ull;
        }
        p.similar[(size_t)gtile * rpad + th] = bits;
    }
    if (IDENT && th <= n) {
        uint32_t* out = p.pair_ident + (size_t)api_row(th, n) * (n + 1);
#pragma unroll
        for (int g = 0; g < kTile; g++) {
            const int32_t tg = gtile * kTile + g;
            if (tg < th) out[api_row(tg, n)] = acc[g];
        }
    }
}

// one workgroup of kGreedyWaves waves
__global__ __launch_bounds__(kGreedyWaves * kLanes) void msa_greedy_kernel(const MsaParams p) {
    __shared__ unsigned long long kept_bits[(SW_MSA_MAX_HITS + 1 + kTile - 1) / kTile];
    __shared__ uint32_t hit[kGreedyWaves][kLanes];
    const int lane = threadIdx.x & (kLanes - 1);
    const int part = threadIdx.x >> 6;
    const int32_t tiles = p.rpad / kTile;
    const int32_t n = p.hits.n;
    const size_t rpad = (size_t)p.rpad;
    int32_t purged = 0;
    for (int32_t b = 0; b < tiles; b++) {
        const int32_t t = b * kTile + lane;
        uint32_t any = 0;
        if (p.similar)
            for (int32_t gt = part; gt < b; gt += kGreedyWaves) any |= (p.similar[(size_t)gt * rpad + t] & kept_bits[gt]) != 0;
        hit[part][lane] = any;
        __syncthreads();
        if (part == 0) {
#pragma unroll
            for (int w = 1; w < kGreedyWaves; w++) any |= hit[w][lane];
            const bool cand = residues_of(p, t) > 0;
            const unsigned long long own = p.similar ? p.similar[(size_t)b * rpad + t] : 0ull;   // bits of earlier rows of this block only
            const unsigned long long open = __ballot(cand && !any);
            unsigned long long kept = 0;   // wave-uniform
            for (int k = 0; k < kTile; k++) {
                const unsigned long long mk = __shfl(own, k, kLanes);
                if ((open >> k & 1ull) && (mk & kept) == 0) kept |= 1ull << k;
            }
            const bool mine = kept >> lane & 1ull;
            if (t <= n) p.keep[api_row(t, n)] = mine ? 1 : 0;
            purged += __popcll(__ballot(cand && !mine));
            if (lane == 0) kept_bits[b] = kept;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *p.purged = purged;
}

}  // namespace swm
