// sw_mask_kernel.hpp — low-complexity masking of a block of subjects: the device side of include/cudasw4_amd_mask.h
// (DESIGN.md §16).  Three launches in stream order over a RANGE of whole subjects (sw_mask.hip cuts a block into ranges that
// fit the caller's scratch); positions and bitmap bits count from the range's first byte, which is a multiple of 4.
//
// Scratch: three bitmaps of one bit per byte of the range, in 64-bit words — lo, trig (window starts, step 3 of the rule)
// and keep (the starts of the runs that hold a trigger, step 5).
//
// 1. flags_kernel — tile-parallel.  A workgroup of 256 threads takes 1 KiB of the range whatever subjects lie in it and
//    stages it plus a halo of 32 bytes in LDS (linear: lane l of a wave reads byte l + j of the wave's 64 + W bytes, four
//    lanes to a dword, 17 consecutive banks at most — conflict-free).  A thread owns the window starts tile + 256 k + tid,
//    k = 0 .. 3, so that the 64 lanes of a wave own the 64 bits of one bitmap word: lo and trig leave the wave as ballots,
//    written by lane 0 with an ordinary store.  Every word of the three bitmaps is written (keep: zero), so the scratch needs
//    no memset.  The subject of a start is found like the shuffle kernel finds it: two scalar binary searches per tile, then
//    a search between the two per thread.  S of a window: the 20 counts n_a live in two 64-bit registers, six bits each
//    (n_a <= 32); one add of a shifted 1 per position, then 20 look-ups of n U[n] in an LDS table — no branch depends on
//    the residues.  A start that is no window of its subject (padding, the last W - 1 positions) has both flags clear, which
//    keeps the runs of neighbouring subjects apart by at least W - 1 >= 3 clear bits.
// 2. resolve_kernel — one lane per subject.  The only step whose reach is unbounded: a run may span a whole subject.  The
//    lane sweeps the words of its subject's starts forward with the carry "this run has triggered" and backward the same;
//    inside a word the fill is one addition (fill_up below).  Words are shared between neighbours (subjects start on
//    multiples of 4, not of 64), so the lane takes only its own bits of a word and ORs its result into keep with a vector
//    atomic; lo and trig are only read.
// 3. apply_kernel — tile-parallel, one dword of output per thread.  Position p is masked iff keep has a bit in
//    (p - W, p]: at most 35 bits for the four positions of a dword, taken from two words.  In place, dwords without a masked
//    byte are not stored.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/cudasw4_amd_mask.h"

namespace swmk {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kStartsPerThread = 4;
constexpr int kTileBytes = kThreads * kStartsPerThread;   // flags: 1 KiB of window starts, 16 bitmap words
constexpr int kHaloBytes = 32;                            // >= SW_MASK_MAX_WINDOW - 1, a multiple of 4
constexpr int kApplyTileBytes = kThreads * 4;
constexpr int kLetters = 20;                              // codes below count; SW_MASK_CODE and above do not

struct Range {
    uint64_t begin;    // byte offset of the range's first subject from the block's start (offsets[first] - offsets[0])
    uint64_t bytes;    // of the range, a multiple of 4
    int32_t first;     // the range's subjects: first .. first + count - 1
    int32_t count;
};

__host__ __device__ inline uint64_t words_of(uint64_t bytes) { return (bytes + 63) / 64; }

// the largest i in [lo, hi] with offsets[i] - base <= b (offsets[lo] - base <= b is the caller's)
__device__ inline int32_t last_at_or_below(const uint64_t* __restrict__ offsets, uint64_t base, int32_t lo, int32_t hi, uint64_t b) {
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] - base <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// true length of subject s: a negative length counts as 0, one over the padded size as that size
__device__ inline uint32_t true_length(const uint64_t* __restrict__ offsets, const int32_t* __restrict__ lengths, int32_t s) {
    const uint64_t sBytes = offsets[s + 1] - offsets[s];
    int32_t len = lengths[s];
    len = len < 0 ? 0 : len;
    return uint64_t(len) > sBytes ? uint32_t(sBytes) : uint32_t(len);
}

__global__ void __launch_bounds__(kThreads) flags_kernel(const int8_t* __restrict__ chars, const uint64_t* __restrict__ offsets,
                                                         const int32_t* __restrict__ lengths, Range r, int32_t window,
                                                         int32_t triggerSum, int32_t extendSum, uint64_t* __restrict__ lo,
                                                         uint64_t* __restrict__ trig, uint64_t* __restrict__ keep) {
    __shared__ uint32_t tileWords[(kTileBytes + kHaloBytes) / 4];
    __shared__ int32_t nU[SW_MASK_MAX_WINDOW + 1];   // n U[n]
    const uint8_t* tileBytes = reinterpret_cast<const uint8_t*>(tileWords);
    const uint64_t base = offsets[0];
    const uint64_t tile = uint64_t(blockIdx.x) * kTileBytes;   // from the range's start
    const int tid = int(threadIdx.x);

    // stage: a dword per thread, the halo by the first threads; bytes behind the range read as code 20
    const uint32_t* src = reinterpret_cast<const uint32_t*>(chars + r.begin);
    constexpr uint32_t kPad = 0x01010101u * uint32_t(SW_MASK_CODE);
    for (int d = tid; d < (kTileBytes + kHaloBytes) / 4; d += kThreads) {
        const uint64_t b = tile + uint64_t(d) * 4;
        tileWords[d] = b < r.bytes ? src[b / 4] : kPad;
    }
    constexpr int32_t kU[SW_MASK_MAX_WINDOW + 1] = {SW_MASK_U_TABLE};
    if (tid <= SW_MASK_MAX_WINDOW) nU[tid] = tid * kU[tid];

    // wave-uniform: the subjects of the tile's first and last dword
    const uint64_t tileLast = (tile + kTileBytes <= r.bytes ? tile + kTileBytes : r.bytes) - 4;
    const int32_t sEnd = r.first + r.count - 1;
    const int32_t sLo = last_at_or_below(offsets, base, r.first, sEnd, r.begin + tile);
    const int32_t sHi = last_at_or_below(offsets, base, sLo, sEnd, r.begin + tileLast);
    __syncthreads();

    const uint64_t words = words_of(r.bytes);
    const int wave = tid / kWave, lane = tid % kWave;
#pragma unroll 1
    for (int k = 0; k < kStartsPerThread; k++) {
        const int local = k * kThreads + tid;
        const uint64_t p = tile + uint64_t(local);
        bool isLo = false, isTrig = false;
        if (p < r.bytes) {
            const int32_t s = last_at_or_below(offsets, base, sLo, sHi, r.begin + p);
            const uint64_t i = r.begin + p - (offsets[s] - base);   // position within the subject
            const uint32_t L = true_length(offsets, lengths, s);
            if (i + uint64_t(window) <= uint64_t(L)) {
                // n_a of the codes 0 .. 9 in c0, 10 .. 19 in c1, six bits each
                uint64_t c0 = 0, c1 = 0;
                for (int j = 0; j < window; j++) {
                    const uint32_t c = tileBytes[local + j];
                    const bool low = c < 10u, high = c >= 10u && c < uint32_t(kLetters);
                    const uint64_t one = uint64_t(1) << (6u * (low ? c : high ? c - 10u : 0u));
                    c0 += low ? one : 0;
                    c1 += high ? one : 0;
                }
                int32_t S = 0;
#pragma unroll
                for (int a = 0; a < 10; a++) {
                    S += nU[(c0 >> (6 * a)) & 63u];
                    S += nU[(c1 >> (6 * a)) & 63u];
                }
                isLo = S >= extendSum;
                isTrig = S >= triggerSum;
            }
        }
        const unsigned long long loBits = __ballot(isLo), trigBits = __ballot(isTrig);
        const uint64_t word = uint64_t(blockIdx.x) * (kTileBytes / 64) + uint64_t(k * (kThreads / kWave) + wave);
        if (lane == 0 && word < words) {
            lo[word] = loBits;
            trig[word] = trigBits;
            keep[word] = 0;
        }
    }
}

// x: a word of lo; seeds: bits of x.  Every bit of x at or above a seed within the seed's run of ones, and in *carry whether
// the fill reached bit 63 (the run may go on in the next word).  Adding the seeds to x ripples a carry from the lowest seed of
// a run to the run's end, flipping every bit on its way except the seeds above it; the clear bit behind the run stops it.
__device__ inline uint64_t fill_up(uint64_t x, uint64_t seeds, uint64_t* carry) {
    const uint64_t y = x + seeds;
    const uint64_t f = ((x ^ y) | seeds) & x;
    *carry = f >> 63;
    return f;
}

// grid: ceil(r.count / kThreads) workgroups, one lane per subject
__global__ void __launch_bounds__(kThreads) resolve_kernel(const uint64_t* __restrict__ offsets, const int32_t* __restrict__ lengths, Range r,
                                                           int32_t window, const uint64_t* __restrict__ lo, const uint64_t* __restrict__ trig,
                                                           uint64_t* __restrict__ keep, unsigned long long* __restrict__ counts) {
    const int32_t t = int32_t(blockIdx.x) * kThreads + int32_t(threadIdx.x);
    bool any = false;
    if (t < r.count) {
        const int32_t s = r.first + t;
        const uint32_t L = true_length(offsets, lengths, s);
        if (L >= uint32_t(window)) {
            // the subject's window starts are the bits [b0, b1] of the range's bitmaps
            const uint64_t b0 = offsets[s] - offsets[0] - r.begin, b1 = b0 + uint64_t(L) - uint64_t(window);
            const uint64_t w0 = b0 / 64, w1 = b1 / 64;
            const uint64_t firstMask = ~uint64_t(0) << (b0 % 64), lastMask = ~uint64_t(0) >> (63 - b1 % 64);
            uint64_t carry = 0;
            for (uint64_t w = w0; w <= w1; w++) {
                const uint64_t own = (w == w0 ? firstMask : ~uint64_t(0)) & (w == w1 ? lastMask : ~uint64_t(0));
                const uint64_t x = lo[w] & own;
                const uint64_t f = fill_up(x, (trig[w] & x) | (carry & x), &carry);
                if (f) { atomicOr(reinterpret_cast<unsigned long long*>(keep + w), (unsigned long long)f); any = true; }
            }
            // backward: the same on the mirrored words, from the last word down (only a subject with a trigger has work)
            carry = 0;
            for (uint64_t w = w1 + 1; any && w-- > w0;) {
                const uint64_t own = (w == w0 ? firstMask : ~uint64_t(0)) & (w == w1 ? lastMask : ~uint64_t(0));
                const uint64_t x = __brevll(lo[w] & own);
                const uint64_t f = __brevll(fill_up(x, (__brevll(trig[w]) & x) | (carry & x), &carry));
                if (f) atomicOr(reinterpret_cast<unsigned long long*>(keep + w), (unsigned long long)f);
            }
        }
    }
    // subjects with a segment: one vector atomic per wave
    if (counts) {
        const unsigned long long n = (unsigned long long)__popcll(__ballot(any));
        if (threadIdx.x % kWave == 0 && n) atomicAdd(counts + 1, n);
    }
}

// grid: ceil(r.bytes / kApplyTileBytes) workgroups, one dword per thread
__global__ void __launch_bounds__(kThreads) apply_kernel(const int8_t* chars, int8_t* out, Range r, int32_t window,
                                                         const uint64_t* __restrict__ keep, int inPlace,
                                                         unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long groupCount;
    if (threadIdx.x == 0) groupCount = 0;
    __syncthreads();
    const uint64_t q0 = (uint64_t(blockIdx.x) * kThreads + threadIdx.x) * 4;   // from the range's start
    uint32_t maskedBytes = 0;   // bit j: position q0 + j is masked
    if (q0 < r.bytes) {
        // bit 63 - d of v: keep of position q0 + 3 - d
        const uint64_t q = q0 + 3, wi = q / 64;
        const uint32_t bi = uint32_t(q % 64);
        uint64_t v = keep[wi] << (63 - bi);
        if (bi < 63 && wi > 0) v |= keep[wi - 1] >> (bi + 1);
        const uint64_t span = (~uint64_t(0)) << (64 - window);   // the window starts that cover one position
#pragma unroll
        for (int j = 0; j < 4; j++)
            maskedBytes |= (v & (span >> (3 - j))) ? (1u << j) : 0u;
        const uint32_t in = *reinterpret_cast<const uint32_t*>(chars + r.begin + q0);
        if (maskedBytes || !inPlace) {
            uint32_t sel = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) sel |= (maskedBytes >> j & 1u) ? (0xffu << (8 * j)) : 0u;
            constexpr uint32_t kX = 0x01010101u * uint32_t(SW_MASK_CODE);
            *reinterpret_cast<uint32_t*>(out + r.begin + q0) = (in & ~sel) | (kX & sel);
        }
    }
    if (counts) {   // covered positions: one vector atomic per workgroup
        unsigned long long n = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) n += (unsigned long long)__popcll(__ballot(maskedBytes >> j & 1u));
        if (threadIdx.x % kWave == 0 && n) atomicAdd(&groupCount, n);
        __syncthreads();
        if (threadIdx.x == 0 && groupCount) atomicAdd(counts, groupCount);
    }
}

}  // namespace swmk
