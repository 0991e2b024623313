// sw_align_kernel.hpp — hit alignment (sw_align_hits): coordinates and CIGAR of one optimal local alignment per
// (query, subject) pair.  DESIGN.md "Hit alignment" has the definition; this file has the three passes over one pair:
//
//   (a) kLocal    the scan's local recurrence over the whole matrix; argmax = the end cell
//   (b) kReverse  the global recurrence (no zero floor) over the reversed prefixes q[qe..0] x s[se..0]; argmax = the start
//   (c) kTrace    the global recurrence over the rectangle q[qs..qe] x s[ss..se], storing 4 direction bits per cell, then
//                 a one-lane walk back that writes the CIGAR and the counts
//
// Both argmaxes take the value first, then the smallest column, then the smallest row (in (b) the reversed coordinates:
// largest subject index, then largest query index), so the wave-wide reduction order does not matter.
//
// Shape: one workgroup = one wave64 per pair, int32 arithmetic (max3 + add, no packing).  Query rows are striped over
// the lanes, kRows rows per lane, 512 rows per stripe; the wave walks the anti-diagonals of a stripe the way dp_step does
// (sw_dp_kernel.hpp): at step t lane l computes column t - l of its rows and hands H / F of its last row to lane l + 1
// with one wave_shr:1 DPP move; lane 0 takes the row above from the stripe border (int2 per column in the pair's
// scratch, written by lane 63 of the stripe before).  The subject letter travels down the lanes the same way.  Letters
// and border values of the next 64 steps are loaded one block ahead (a subject dword serves 4 letters) and read out
// with v_readlane, so the step loop never waits on global memory.  The substitution rows live in LDS.
//
// Direction bits of (c): kRows x 4 bits = one dword per lane and step, stored at [stripe][step][lane], so the 64
// stores of one step are contiguous.  Per cell: bits 0-1 where H came from (0 diagonal, 1 E, 2 F; ties in that order),
// bit 2 E extended (else opened), bit 3 F extended.  Only vector stores are used.
//
// PSSM form (sw_align_hits_pssm, DESIGN.md "Hit alignment of PSSM queries"): the substitution score of row i is
// pssm[i][s_j] in place of M[q_i][s_j].  dp_pass<MODE, true> keeps the step loop and takes the scores from an LDS tile of
// the stripe's 512 PSSM rows, laid out [row-in-lane r][letter][lane] in dwords: lane l reads word (r * 21 + letter) * 64
// + l, which lies in bank l whatever letters the 64 lanes look up.  The tile is reloaded at the start of every stripe
// (load_tile); the letter form is the template's other instantiation and compiles to what it was before the template.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "../../include/cudasw4_amd.h"
#include "../../include/cudasw4_amd_hsps.h"

namespace swa {

constexpr int kLanes = 64;
constexpr int kRows = 8;                  // rows per lane: 8 x 4 direction bits = one dword per lane and step
constexpr int kStripe = kLanes * kRows;   // query rows per stripe
constexpr int kLetters = 21;              // subject alphabet (dbdata codes)
constexpr int kMatrixRows = 26;           // 25 query letters + the padding row (sw_set_matrix's internal form)
constexpr int kTileWords = kRows * kLetters * kLanes;   // PSSM form: one stripe's rows in LDS, 43 008 bytes
constexpr int32_t kNeg = -(1 << 30);      // E / F before any gap
// The global passes clamp H at kFloor.  A path whose prefix went below it cannot climb back to a score >= 0 within
// 2^20 query rows (int8 substitution scores), so no cell an optimal alignment uses ever differs from the exact DP.
constexpr int32_t kFloor = -(1 << 29);

enum Mode { kLocal = 0, kReverse = 1, kTrace = 2 };

struct Best {
    int32_t v, j, i;   // value, column (0-based), row (0-based)
};

__device__ __forceinline__ bool better(const Best& a, const Best& b) {
    return a.v > b.v || (a.v == b.v && (a.j < b.j || (a.j == b.j && a.i < b.i)));
}

// one pass over rows x cols.  Row i (0-based) is query code q[dir * i], column j is subject letter s[dir * j].
// PSSM form: row i is the PSSM row at q + dir * i * kLetters, and mrows is not used.
struct Pass {
    const int8_t* q;
    const int8_t* s;
    int32_t rows, cols;
    int32_t mrows;        // query codes must be < mrows (others are scored as code 0: never reached with checked input)
    int32_t gop, gex;
    int2* border;         // cols entries (multi-stripe passes)
    uint32_t* trace;      // kTrace: ceil(rows / kStripe) * (cols + kLanes - 1) * kLanes dwords
};

// the vetoed form of a pass (sw_align_hsps, DESIGN.md "Several alignments per hit"): the diagonal move into a cell that
// is an aligned pair of one of the pair's `nprev` earlier alignments is not available.  used[a * upitch + i] is the
// subject column alignment a pairs with query row i (both in the pair's own coordinates), or -1; the pass's row i is
// the pair's row org_r + dir * i and its column j the pair's column org_c + dir * j.
struct VetoPass : Pass {
    const int32_t* used;
    int32_t nprev, upitch;
    int32_t org_r, org_c;
};

__device__ __forceinline__ int32_t shr1(int32_t lane0, int32_t src) {
    // wave_shr:1 — lane l gets src of lane l - 1, lane 0 keeps `lane0`
    return __builtin_amdgcn_update_dpp(lane0, src, 0x138, 0xf, 0xf, false);
}

__device__ __forceinline__ int32_t imax(int32_t a, int32_t b) { return a > b ? a : b; }

// PSSM form: rows [k * kStripe, k * kStripe + nrows) of the pass into the tile, the other rows of the tile zero.  The
// stripe's rows are one contiguous piece of the row-major array (in kReverse it ends at the pass's row 0); the wave reads
// it as aligned dwords, 64 consecutive ones per load, and scatters the four scores of each.  A dword that holds a byte of
// the piece lies in memory the piece's pages cover, so the bytes around the piece are read but never used.
template <int MODE>
__device__ __forceinline__ void load_tile(const Pass& ps, const int k, int32_t* tile, const int lane) {
    constexpr int kTileBytes = kStripe * kLetters;
    const int32_t left = ps.rows - k * kStripe;
    const int32_t nrows = left < kStripe ? left : kStripe;
    const int32_t nbytes = nrows * kLetters;
    const int8_t* lo = MODE == kReverse ? ps.q - ((int64_t)k * kStripe + nrows - 1) * kLetters : ps.q + (int64_t)k * kStripe * kLetters;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(lo);
    const int32_t shift = (int32_t)(addr & 3);
    const uint32_t* words = reinterpret_cast<const uint32_t*>(addr & ~uintptr_t(3));
    for (int32_t w = lane; w < (kTileBytes + 3) / 4 + 1; w += kLanes) {
        const int32_t e0 = 4 * w - shift;   // byte of the piece the dword starts with
        const uint32_t v = e0 < nbytes ? words[w] : 0u;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int32_t e = e0 + b;
            if (e < 0 || e >= kTileBytes) continue;
            const int32_t m = e / kLetters, c = e - m * kLetters;
            const bool valid = e < nbytes;
            const int32_t n = (MODE == kReverse && valid) ? nrows - 1 - m : m;   // row of the stripe
            tile[((n % kRows) * kLetters + c) * kLanes + n / kRows] = valid ? (int32_t)(int8_t)(v >> (8 * b)) : 0;
        }
    }
}

// lds_m: the letter form's substitution rows (kMatrixRows x kLetters), or the PSSM form's tile (kTileWords)
//
// VETO (dp_pass<MODE, PSSM, true>, a VetoPass): every lane reads the used columns of its rows once per stripe and keeps, for
// the 64 steps of a block and each of its rows, one bit "the column of this step is paired with this row already", built
// one block ahead from registers; per group of 8 steps "some lane has such a bit" is wave-uniform (ballots, SGPRs), and a
// step of a group without one runs the plain row loop.
template <int MODE, bool PSSM = false, bool VETO = false>
__device__ Best dp_pass(const std::conditional_t<VETO, VetoPass, Pass>& ps, int32_t* lds_m, const int lane) {
    constexpr bool kGlobal = MODE != kLocal;
    constexpr int dir = MODE == kReverse ? -1 : 1;
    const int32_t gop = ps.gop, gex = ps.gex;
    const int32_t floor = kGlobal ? kFloor : 0;
    const int nst = (ps.rows + kStripe - 1) / kStripe;
    const int64_t pitch = (int64_t)ps.cols + kLanes - 1;
    // H in column 0 of row n / in row 0 of column n (n >= 1 cells of gap; n = 0: the corner)
    auto edge = [&](int64_t n) -> int32_t {
        if (!kGlobal || n == 0) return 0;
        const int64_t v = gop + (n - 1) * (int64_t)gex;
        return v < floor ? floor : (int32_t)v;
    };
    Best best{kGlobal ? INT_MIN : 0, INT_MAX, INT_MAX};
    for (int k = 0; k < nst; k++) {
        if (k) __syncthreads();   // the border lane 63 wrote is visible to lane 0 (PSSM form: and the tile is free)
        if constexpr (PSSM) {
            load_tile<MODE>(ps, k, lds_m, lane);
            __syncthreads();      // the tile is complete
        }
        const int32_t row0 = k * kStripe + lane * kRows;
        const int32_t nvalid = ps.rows - row0 < 0 ? 0 : (ps.rows - row0 > kRows ? kRows : ps.rows - row0);
        int32_t qo[kRows], Hl[kRows], E[kRows];
#pragma unroll
        for (int r = 0; r < kRows; r++) {
            if constexpr (PSSM) {
                qo[r] = r * kLetters * kLanes + lane;   // + letter * kLanes: the word of (row r of this lane, letter)
            } else {
                int32_t c = r < nvalid ? ps.q[dir * (int64_t)(row0 + r)] : 0;
                c = (unsigned)c < (unsigned)ps.mrows ? c : 0;
                qo[r] = c * kLetters;
            }
            Hl[r] = edge(row0 + r + 1);
            E[r] = kNeg;
        }
        int32_t diag_in = edge(row0);   // H(row above, column 0)
        int32_t lastH = 0, lastF = kNeg, sc = 0;
        const int32_t active = (ps.rows - k * kStripe + kRows - 1) / kRows;
        const int32_t steps = ps.cols + (active < kLanes ? active : kLanes) - 1;
        Best sb{kGlobal ? INT_MIN : 0, 0, 0};
        // step t of the block [t0, t0 + 64) reads lane t - t0's letter and border values
        auto load_block = [&](int32_t t0, int32_t& letter, int32_t& bh, int32_t& bf) {
            const int32_t t = t0 + lane;
            letter = 0;
            bh = 0;
            bf = kNeg;
            if (t < ps.cols) {
                const int8_t* a = ps.s + dir * (int64_t)t;
                const uintptr_t addr = reinterpret_cast<uintptr_t>(a);
                const uint32_t w = *reinterpret_cast<const uint32_t*>(addr & ~uintptr_t(3));
                const int32_t c = (int32_t)((w >> (8 * (addr & 3))) & 0xffu);
                letter = c > kLetters - 1 ? kLetters - 1 : c;
                if constexpr (PSSM) letter *= kLanes;   // travels down the lanes as the tile offset of its column
                if (k == 0) {
                    bh = edge(t + 1);
                } else {
                    const int2 v = ps.border[t];
                    bh = v.x;
                    bf = v.y;
                }
            }
        };
        // VETO: the lane's used columns, one per earlier alignment and row, read once per stripe and kept in registers: the
        // column in the pass's frame plus the lane number = the step in which the lane meets it (kNoStep: none)
        constexpr int kMaxPrev = VETO ? SW_MAX_HSPS - 1 : 1;
        constexpr int32_t kNoStep = -(1 << 30);
        [[maybe_unused]] int32_t ustep[kMaxPrev][kRows];
        if constexpr (VETO) {
#pragma unroll
            for (int a = 0; a < kMaxPrev; a++) {
                if (a < ps.nprev) {
                    const int32_t* urow = ps.used + (int64_t)a * ps.upitch + ps.org_r + dir * (int64_t)row0;
#pragma unroll
                    for (int r = 0; r < kRows; r++) {
                        const int32_t c = r < nvalid ? urow[dir * r] : -1;
                        ustep[a][r] = c >= 0 ? dir * (c - ps.org_c) + lane : kNoStep;
                    }
                }
            }
        }
        // bit u of m[r] = step t0 + u of this lane is a used pair of its row r; bit g of `any` = some lane has a used pair in
        // the steps [t0 + 8 g, t0 + 8 g + 8) (8 ballots: wave-uniform, in SGPRs, no LDS or memory traffic)
        [[maybe_unused]] auto load_veto = [&](int32_t t0, uint64_t (&m)[kRows], uint32_t& any) {
            if constexpr (VETO) {
#pragma unroll
                for (int r = 0; r < kRows; r++) m[r] = 0;
#pragma unroll
                for (int a = 0; a < kMaxPrev; a++) {
                    if (a < ps.nprev) {
#pragma unroll
                        for (int r = 0; r < kRows; r++) {
                            const int32_t u = ustep[a][r] - t0;
                            if ((uint32_t)u < (uint32_t)kLanes) m[r] |= uint64_t(1) << u;
                        }
                    }
                }
                uint64_t w = 0;
#pragma unroll
                for (int r = 0; r < kRows; r++) w |= m[r];
                any = 0;
#pragma unroll
                for (int g = 0; g < 8; g++)
                    if (__builtin_amdgcn_ballot_w64(((w >> (8 * g)) & 0xffu) != 0) != 0) any |= 1u << g;
            }
        };
        int32_t nl, nbh, nbf;
        load_block(0, nl, nbh, nbf);
        [[maybe_unused]] uint64_t nvm[kRows], vm[kRows];
        [[maybe_unused]] uint32_t nany = 0, any = 0;
        if constexpr (VETO) load_veto(0, nvm, nany);
        for (int32_t t0 = 0; t0 < steps; t0 += kLanes) {
            const int32_t bl = nl, bh = nbh, bf = nbf;
            if constexpr (VETO) {
#pragma unroll
                for (int r = 0; r < kRows; r++) vm[r] = nvm[r];
                any = nany;
            }
            if (t0 + kLanes < steps) {
                load_block(t0 + kLanes, nl, nbh, nbf);
                if constexpr (VETO) load_veto(t0 + kLanes, nvm, nany);
            }
            const int32_t tend = steps - t0 < kLanes ? steps - t0 : kLanes;
            for (int32_t u = 0; u < tend; u++) {
                const int32_t t = t0 + u;
                sc = shr1(__builtin_amdgcn_readlane(bl, u), sc);
                const int32_t uh = shr1(__builtin_amdgcn_readlane(bh, u), lastH);
                const int32_t uf = shr1(__builtin_amdgcn_readlane(bf, u), lastF);
                const int32_t j = t - lane;
                if (j >= 0 && j < ps.cols) {
                    int32_t diag = diag_in;
                    diag_in = uh;
                    int32_t hu = uh, fu = uf;
                    uint32_t bits = 0;
                    if constexpr (!VETO) {   // (left as it stood, not shared with the branch below: DESIGN.md §14 on the ISA)
#pragma unroll
                    for (int r = 0; r < kRows; r++) {
                        const int32_t eo = Hl[r] + gop, ee = E[r] + gex;
                        const int32_t fo = hu + gop, fe = fu + gex;
                        const int32_t e = imax(eo, ee), f = imax(fo, fe);
                        const int32_t dm = diag + lds_m[qo[r] + sc];
                        const int32_t h = imax(imax(dm, e), imax(f, floor));
                        if constexpr (MODE == kTrace) {
                            const uint32_t src = h == dm ? 0u : (h == e ? 1u : 2u);
                            bits |= (src | (uint32_t)(ee > eo) << 2 | (uint32_t)(fe > fo) << 3) << (4 * r);
                        } else {
                            if (r < nvalid && h > sb.v) sb = Best{h, j, row0 + r};
                        }
                        diag = Hl[r];
                        Hl[r] = h;
                        E[r] = e;
                        hu = h;
                        fu = f;
                    }
                    } else {
                        // the same row loop twice: the steps in which some lane has a used pair take the copy that tests
                        // the lane's bits, all others the plain one (the branch is wave-uniform: `any` is in SGPRs)
                        auto row_loop = [&](auto vetoed) {
#pragma unroll
                            for (int r = 0; r < kRows; r++) {
                                const int32_t eo = Hl[r] + gop, ee = E[r] + gex;
                                const int32_t fo = hu + gop, fe = fu + gex;
                                const int32_t e = imax(eo, ee), f = imax(fo, fe);
                                int32_t dm = diag + lds_m[qo[r] + sc];
                                if constexpr (decltype(vetoed)::value) dm = (vm[r] >> u & 1) ? kNeg : dm;   // kNeg < floor <= h: never h == dm
                                const int32_t h = imax(imax(dm, e), imax(f, floor));
                                if constexpr (MODE == kTrace) {
                                    const uint32_t src = h == dm ? 0u : (h == e ? 1u : 2u);
                                    bits |= (src | (uint32_t)(ee > eo) << 2 | (uint32_t)(fe > fo) << 3) << (4 * r);
                                } else {
                                    if (r < nvalid && h > sb.v) sb = Best{h, j, row0 + r};
                                }
                                diag = Hl[r];
                                Hl[r] = h;
                                E[r] = e;
                                hu = h;
                                fu = f;
                            }
                        };
                        if (any >> (u >> 3) & 1) row_loop(std::true_type{}); else row_loop(std::false_type{});
                    }
                    lastH = hu;
                    lastF = fu;
                    if constexpr (MODE == kTrace) ps.trace[((int64_t)k * pitch + t) * kLanes + lane] = bits;
                    if (lane == kLanes - 1 && k + 1 < nst) ps.border[j] = make_int2(hu, fu);
                }
            }
        }
        if (MODE != kTrace && better(sb, best)) best = sb;
    }
    if constexpr (MODE != kTrace) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const Best o{__shfl_xor(best.v, off), __shfl_xor(best.j, off), __shfl_xor(best.i, off)};
            if (better(o, best)) best = o;
        }
    }
    return best;
}

// PSSM form: `matrix` is the PSSM (qlen x kLetters, row-major), `query` the consensus codes or null, mrows is not used
struct AlignParams {
    const int8_t* query;
    int32_t qlen;
    const int8_t* chars;
    const uint64_t* offsets;
    const int32_t* lengths;
    int32_t max_len;
    const int8_t* matrix;   // (mrows) x 21, the context's internal form
    int32_t mrows;
    int32_t gop, gex;
    const int32_t* expected;
    sw_align_result* results;
    uint32_t* cigar;
    const int64_t* cigar_offsets;
    int32_t first;          // first pair of this launch
    char* temp;             // one slot per workgroup
    size_t slot_bytes, border_bytes, trace_bytes;
};

__device__ __forceinline__ void load_matrix(const AlignParams& p, int32_t* lds_m) {
    for (int i = threadIdx.x; i < kMatrixRows * kLetters; i += kLanes)
        lds_m[i] = i < p.mrows * kLetters ? (int32_t)p.matrix[i] : 0;
    __syncthreads();
}

// the LDS of a kernel and what fills it before the passes: the table (letter form) or nothing (the passes load the tile)
template <bool PSSM>
constexpr int kLdsWords = PSSM ? kTileWords : kMatrixRows * kLetters;

template <bool PSSM>
__device__ __forceinline__ void load_scores(const AlignParams& p, int32_t* lds_m) {
    if constexpr (!PSSM) load_matrix(p, lds_m);
}

// row i of the query as a pass sees it
template <bool PSSM>
__device__ __forceinline__ const int8_t* query_row(const AlignParams& p, int32_t i) {
    return PSSM ? p.matrix + (int64_t)i * kLetters : p.query + i;
}

// PSSM form: the consensus code of position i — the caller's, or the lowest code < 20 with the largest score
__device__ __forceinline__ int32_t consensus_code(const AlignParams& p, int32_t i) {
    if (p.query) return p.query[i];
    const int8_t* row = p.matrix + (int64_t)i * kLetters;
    int32_t best = 0;
    for (int32_t c = 1; c < 20; c++)
        if (row[c] > row[best]) best = c;
    return best;
}

// (a): score, end, status
template <bool PSSM>
__global__ __launch_bounds__(kLanes) void align_end_kernel(AlignParams p) {
    __shared__ int32_t lds_m[kLdsWords<PSSM>];
    load_scores<PSSM>(p, lds_m);
    const int lane = threadIdx.x;
    const int32_t pair = p.first + blockIdx.x;
    const int32_t len = p.lengths[pair];
    sw_align_result* res = p.results + pair;
    if (len > p.max_len) {
        if (lane == 0) *res = sw_align_result{0, SW_ALIGN_BAD_LENGTH, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0};
        return;
    }
    Best b{0, -1, -1};
    if (len > 0 && p.qlen > 0) {
        char* slot = p.temp + (size_t)blockIdx.x * p.slot_bytes;
        const Pass ps{query_row<PSSM>(p, 0), p.chars + (p.offsets[pair] - p.offsets[0]), p.qlen, len, p.mrows, p.gop, p.gex,
                      reinterpret_cast<int2*>(slot), nullptr};
        b = dp_pass<kLocal, PSSM>(ps, lds_m, lane);
    }
    if (lane == 0) {
        const int32_t S = b.v;
        int32_t status = S > 0 ? SW_ALIGN_OK : SW_ALIGN_EMPTY;
        if (p.expected && p.expected[pair] != S) status = SW_ALIGN_SCORE_MISMATCH;
        const bool at = S > 0;
        *res = sw_align_result{S, status, -1, at ? b.i + 1 : -1, -1, at ? b.j + 1 : -1, 0, 0, 0, 0, 0, 0,
                               p.cigar_offsets ? p.cigar_offsets[pair] : 0};
    }
}

// (b): start
template <bool PSSM>
__global__ __launch_bounds__(kLanes) void align_start_kernel(AlignParams p) {
    __shared__ int32_t lds_m[kLdsWords<PSSM>];
    load_scores<PSSM>(p, lds_m);
    const int lane = threadIdx.x;
    const int32_t pair = p.first + blockIdx.x;
    sw_align_result* res = p.results + pair;
    const int32_t status = res->status, S = res->score;
    if ((status != SW_ALIGN_OK && status != SW_ALIGN_SCORE_MISMATCH) || S <= 0) return;
    const int32_t qe = res->q_end - 1, se = res->s_end - 1;
    char* slot = p.temp + (size_t)blockIdx.x * p.slot_bytes;
    const Pass ps{query_row<PSSM>(p, qe), p.chars + (p.offsets[pair] - p.offsets[0]) + se, qe + 1, se + 1, p.mrows, p.gop, p.gex,
                  reinterpret_cast<int2*>(slot), nullptr};
    const Best b = dp_pass<kReverse, PSSM>(ps, lds_m, lane);
    if (lane == 0) {
        res->q_begin = qe - b.i;
        res->s_begin = se - b.j;
    }
}

// (c): direction bits of the rectangle, then lane 0 walks back from its far corner
// (The walk and the CIGAR emission stand a second time in hsp_trace_kernel below, with the used-pair store added; this kernel
// stays as it is so that its code does too — DESIGN.md "Several alignments per hit".  A fix to one is a fix to both.)
template <bool PSSM>
__global__ __launch_bounds__(kLanes) void align_trace_kernel(AlignParams p) {
    __shared__ int32_t lds_m[kLdsWords<PSSM>];
    load_scores<PSSM>(p, lds_m);
    const int lane = threadIdx.x;
    const int32_t pair = p.first + blockIdx.x;
    sw_align_result* res = p.results + pair;
    if (res->status != SW_ALIGN_OK) return;
    const int32_t qs = res->q_begin, ss = res->s_begin;
    const int32_t rows = res->q_end - qs, cols = res->s_end - ss;
    const int64_t pitch = (int64_t)cols + kLanes - 1;
    const int64_t nst = (rows + kStripe - 1) / kStripe;
    if ((uint64_t)(nst * pitch * kLanes * 4) > p.trace_bytes) {
        if (lane == 0) res->status = SW_ALIGN_NO_TRACE;
        return;
    }
    char* slot = p.temp + (size_t)blockIdx.x * p.slot_bytes;
    const int8_t* q = query_row<PSSM>(p, qs);
    const int8_t* s = p.chars + (p.offsets[pair] - p.offsets[0]) + ss;
    uint32_t* trace = reinterpret_cast<uint32_t*>(slot + p.border_bytes);
    const Pass ps{q, s, rows, cols, p.mrows, p.gop, p.gex, reinterpret_cast<int2*>(slot), trace};
    dp_pass<kTrace, PSSM>(ps, lds_m, lane);
    __syncthreads();   // every lane's direction bits are visible to lane 0
    if (lane != 0) return;
    auto nib = [&](int32_t i, int32_t j) -> uint32_t {   // 0-based cell of the rectangle
        const int32_t k = i / kStripe, l = (i % kStripe) / kRows, r = i % kRows;
        return (trace[((int64_t)k * pitch + j + l) * kLanes + l] >> (4 * r)) & 15u;
    };
    const int64_t c0 = p.cigar_offsets[pair];
    const int64_t cap = p.cigar_offsets[pair + 1] - c0;
    uint32_t* out = p.cigar + c0;
    int64_t nruns = 0;
    uint32_t run_op = 0, run_len = 0;
    int32_t ids = 0, mis = 0, opens = 0, gcols = 0;
    auto emit = [&](uint32_t op) {
        if (op != run_op) {
            if (run_len) {
                if (nruns < cap) out[nruns] = run_len << 4 | run_op;
                nruns++;
            }
            if (op == SW_CIGAR_I || op == SW_CIGAR_D) opens++;
            run_op = op;
            run_len = 0;
        }
        run_len++;
    };
    int32_t i = rows, j = cols, state = 0;
    while (i > 0 && j > 0) {
        const uint32_t d = nib(i - 1, j - 1);
        if (state == 0) {
            if ((d & 3u) == 0) {
                if constexpr (PSSM) {
                    const int32_t b = s[j - 1];
                    if (b >= 0 && b < 20 && b == consensus_code(p, qs + i - 1)) { emit(SW_CIGAR_EQ); ids++; } else { emit(SW_CIGAR_X); mis++; }
                } else {
                    const int8_t a = q[i - 1], b = s[j - 1];
                    if (a == b && a >= 0 && a < 20) { emit(SW_CIGAR_EQ); ids++; } else { emit(SW_CIGAR_X); mis++; }
                }
                i--;
                j--;
            } else {
                state = (int32_t)(d & 3u);
            }
        } else if (state == 1) {
            emit(SW_CIGAR_D);
            gcols++;
            state = (d >> 2 & 1u) ? 1 : 0;
            j--;
        } else {
            emit(SW_CIGAR_I);
            gcols++;
            state = (d >> 3 & 1u) ? 2 : 0;
            i--;
        }
    }
    for (; i > 0; i--) { emit(SW_CIGAR_I); gcols++; }
    for (; j > 0; j--) { emit(SW_CIGAR_D); gcols++; }
    if (run_len) {
        if (nruns < cap) out[nruns] = run_len << 4 | run_op;
        nruns++;
    }
    if (nruns > cap) {
        res->status = SW_ALIGN_NO_TRACE;
        return;
    }
    for (int64_t a = 0, b = nruns - 1; a < b; a++, b--) {   // runs were written last-first
        const uint32_t x = out[a];
        out[a] = out[b];
        out[b] = x;
    }
    res->columns = ids + mis + gcols;
    res->identities = ids;
    res->mismatches = mis;
    res->gap_opens = opens;
    res->gap_columns = gcols;
    res->cigar_len = (int32_t)nruns;
}

// ---- several alignments per hit (sw_align_hsps, include/cudasw4_amd_hsps.h; DESIGN.md "Several alignments per hit") ----
//
// Round k of a pair computes its alignment k into record pair * max_hsps + k: the three phases above, with the diagonal move
// into the aligned pairs of alignments 0 .. k-1 vetoed (VETO = k > 0; round 0 runs the plain passes).  The pairs live in
// the pair's scratch behind the direction bits: row a of qlen int32 = the subject column alignment a pairs with each
// query row, or -1, filled and written by round a's trace kernel (lane 0's walk, ordinary stores).  The last round's pairs
// are never read and not recorded.
struct HspParams {
    AlignParams a;          // results: n * max_hsps records; cigar_offsets: n * max_hsps + 1
    int32_t round, max_hsps, min_score;
    size_t used_off;        // the used-pair rows within a pair's slot
};

__device__ __forceinline__ int32_t* used_rows(const HspParams& hp, char* slot) { return reinterpret_cast<int32_t*>(slot + hp.used_off); }

// (a): score, end, status; rounds behind a slot that is not OK write the terminal record and return
template <bool PSSM, bool VETO>
__global__ __launch_bounds__(kLanes) void hsp_end_kernel(HspParams hp) {
    const AlignParams& p = hp.a;
    __shared__ int32_t lds_m[kLdsWords<PSSM>];
    load_scores<PSSM>(p, lds_m);
    const int lane = threadIdx.x;
    const int32_t pair = p.first + blockIdx.x;
    const int64_t rec = (int64_t)pair * hp.max_hsps + hp.round;
    sw_align_result* res = p.results + rec;
    const int64_t coff = p.cigar_offsets[rec];
    if constexpr (VETO) {
        const int32_t prev = res[-1].status;
        if (prev != SW_ALIGN_OK) {
            // nothing follows an empty slot; nothing can be defined behind an alignment whose pairs are unknown
            const int32_t st = prev == SW_ALIGN_EMPTY ? SW_ALIGN_EMPTY : SW_ALIGN_NOT_COMPUTED;
            if (lane == 0) *res = sw_align_result{0, st, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0, coff};
            return;
        }
    }
    const int32_t len = p.lengths[pair];
    if (len > p.max_len) {
        if (lane == 0) *res = sw_align_result{0, SW_ALIGN_BAD_LENGTH, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0};
        return;
    }
    Best b{0, -1, -1};
    if (len > 0 && p.qlen > 0) {
        char* slot = p.temp + (size_t)blockIdx.x * p.slot_bytes;
        const Pass ps{query_row<PSSM>(p, 0), p.chars + (p.offsets[pair] - p.offsets[0]), p.qlen, len, p.mrows, p.gop, p.gex,
                      reinterpret_cast<int2*>(slot), nullptr};
        if constexpr (VETO) {
            const VetoPass vp{ps, used_rows(hp, slot), hp.round, p.qlen, 0, 0};
            b = dp_pass<kLocal, PSSM, true>(vp, lds_m, lane);
        } else {
            b = dp_pass<kLocal, PSSM>(ps, lds_m, lane);
        }
    }
    if (lane == 0) {
        int32_t S = b.v;
        int32_t status = S > 0 ? SW_ALIGN_OK : SW_ALIGN_EMPTY;
        if constexpr (VETO) {
            if (S < hp.min_score) {   // (min_score >= 1) the slot and everything behind it is empty
                S = 0;
                status = SW_ALIGN_EMPTY;
            }
        } else {
            if (p.expected && p.expected[pair] != S) status = SW_ALIGN_SCORE_MISMATCH;
        }
        const bool at = S > 0;
        *res = sw_align_result{S, status, -1, at ? b.i + 1 : -1, -1, at ? b.j + 1 : -1, 0, 0, 0, 0, 0, 0, coff};
    }
}

// (b): start
template <bool PSSM, bool VETO>
__global__ __launch_bounds__(kLanes) void hsp_start_kernel(HspParams hp) {
    const AlignParams& p = hp.a;
    __shared__ int32_t lds_m[kLdsWords<PSSM>];
    load_scores<PSSM>(p, lds_m);
    const int lane = threadIdx.x;
    const int32_t pair = p.first + blockIdx.x;
    sw_align_result* res = p.results + ((int64_t)pair * hp.max_hsps + hp.round);
    const int32_t status = res->status, S = res->score;
    if ((status != SW_ALIGN_OK && status != SW_ALIGN_SCORE_MISMATCH) || S <= 0) return;
    const int32_t qe = res->q_end - 1, se = res->s_end - 1;
    char* slot = p.temp + (size_t)blockIdx.x * p.slot_bytes;
    const Pass ps{query_row<PSSM>(p, qe), p.chars + (p.offsets[pair] - p.offsets[0]) + se, qe + 1, se + 1, p.mrows, p.gop, p.gex,
                  reinterpret_cast<int2*>(slot), nullptr};
    Best b;
    if constexpr (VETO) {
        const VetoPass vp{ps, used_rows(hp, slot), hp.round, p.qlen, qe, se};
        b = dp_pass<kReverse, PSSM, true>(vp, lds_m, lane);
    } else {
        b = dp_pass<kReverse, PSSM>(ps, lds_m, lane);
    }
    if (lane == 0) {
        res->q_begin = qe - b.i;
        res->s_begin = se - b.j;
    }
}

// (c): direction bits, the walk back, and the alignment's pairs for the rounds behind it
// (The walk and the CIGAR emission are align_trace_kernel's, copied: only the record index, the fill of the used-pair row and
// the store at every diagonal step differ.  A fix to one is a fix to both; hsp_end_kernel / hsp_start_kernel likewise mirror
// align_end_kernel / align_start_kernel.)
template <bool PSSM, bool VETO>
__global__ __launch_bounds__(kLanes) void hsp_trace_kernel(HspParams hp) {
    const AlignParams& p = hp.a;
    __shared__ int32_t lds_m[kLdsWords<PSSM>];
    load_scores<PSSM>(p, lds_m);
    const int lane = threadIdx.x;
    const int32_t pair = p.first + blockIdx.x;
    const int64_t rec = (int64_t)pair * hp.max_hsps + hp.round;
    sw_align_result* res = p.results + rec;
    if (res->status != SW_ALIGN_OK) return;
    const int32_t qs = res->q_begin, ss = res->s_begin;
    const int32_t rows = res->q_end - qs, cols = res->s_end - ss;
    const int64_t pitch = (int64_t)cols + kLanes - 1;
    const int64_t nst = (rows + kStripe - 1) / kStripe;
    if ((uint64_t)(nst * pitch * kLanes * 4) > p.trace_bytes) {
        if (lane == 0) res->status = SW_ALIGN_NO_TRACE;
        return;
    }
    char* slot = p.temp + (size_t)blockIdx.x * p.slot_bytes;
    const int8_t* q = query_row<PSSM>(p, qs);
    const int8_t* s = p.chars + (p.offsets[pair] - p.offsets[0]) + ss;
    uint32_t* trace = reinterpret_cast<uint32_t*>(slot + p.border_bytes);
    const bool record = hp.round + 1 < hp.max_hsps;
    int32_t* urow = used_rows(hp, slot) + (int64_t)hp.round * p.qlen;
    if (record)
        for (int32_t i = lane; i < p.qlen; i += kLanes) urow[i] = -1;
    const Pass ps{q, s, rows, cols, p.mrows, p.gop, p.gex, reinterpret_cast<int2*>(slot), trace};
    if constexpr (VETO) {
        const VetoPass vp{ps, used_rows(hp, slot), hp.round, p.qlen, qs, ss};
        dp_pass<kTrace, PSSM, true>(vp, lds_m, lane);
    } else {
        dp_pass<kTrace, PSSM>(ps, lds_m, lane);
    }
    __syncthreads();   // every lane's direction bits (and the fill of the used-pair row) are visible to lane 0
    if (lane != 0) return;
    auto nib = [&](int32_t i, int32_t j) -> uint32_t {   // 0-based cell of the rectangle
        const int32_t k = i / kStripe, l = (i % kStripe) / kRows, r = i % kRows;
        return (trace[((int64_t)k * pitch + j + l) * kLanes + l] >> (4 * r)) & 15u;
    };
    const int64_t c0 = p.cigar_offsets[rec];
    const int64_t cap = p.cigar_offsets[rec + 1] - c0;
    uint32_t* out = p.cigar + c0;
    int64_t nruns = 0;
    uint32_t run_op = 0, run_len = 0;
    int32_t ids = 0, mis = 0, opens = 0, gcols = 0;
    auto emit = [&](uint32_t op) {
        if (op != run_op) {
            if (run_len) {
                if (nruns < cap) out[nruns] = run_len << 4 | run_op;
                nruns++;
            }
            if (op == SW_CIGAR_I || op == SW_CIGAR_D) opens++;
            run_op = op;
            run_len = 0;
        }
        run_len++;
    };
    int32_t i = rows, j = cols, state = 0;
    while (i > 0 && j > 0) {
        const uint32_t d = nib(i - 1, j - 1);
        if (state == 0) {
            if ((d & 3u) == 0) {
                if constexpr (PSSM) {
                    const int32_t b = s[j - 1];
                    if (b >= 0 && b < 20 && b == consensus_code(p, qs + i - 1)) { emit(SW_CIGAR_EQ); ids++; } else { emit(SW_CIGAR_X); mis++; }
                } else {
                    const int8_t a = q[i - 1], b = s[j - 1];
                    if (a == b && a >= 0 && a < 20) { emit(SW_CIGAR_EQ); ids++; } else { emit(SW_CIGAR_X); mis++; }
                }
                if (record) urow[qs + i - 1] = ss + j - 1;
                i--;
                j--;
            } else {
                state = (int32_t)(d & 3u);
            }
        } else if (state == 1) {
            emit(SW_CIGAR_D);
            gcols++;
            state = (d >> 2 & 1u) ? 1 : 0;
            j--;
        } else {
            emit(SW_CIGAR_I);
            gcols++;
            state = (d >> 3 & 1u) ? 2 : 0;
            i--;
        }
    }
    for (; i > 0; i--) { emit(SW_CIGAR_I); gcols++; }
    for (; j > 0; j--) { emit(SW_CIGAR_D); gcols++; }
    if (run_len) {
        if (nruns < cap) out[nruns] = run_len << 4 | run_op;
        nruns++;
    }
    if (nruns > cap) {
        res->status = SW_ALIGN_NO_TRACE;
        return;
    }
    for (int64_t a = 0, b = nruns - 1; a < b; a++, b--) {   // runs were written last-first
        const uint32_t x = out[a];
        out[a] = out[b];
        out[b] = x;
    }
    res->columns = ids + mis + gcols;
    res->identities = ids;
    res->mismatches = mis;
    res->gap_opens = opens;
    res->gap_columns = gcols;
    res->cigar_len = (int32_t)nruns;
}


}  // namespace swa
