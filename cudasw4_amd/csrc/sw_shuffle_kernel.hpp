// sw_shuffle_kernel.hpp — replicas of a block of subjects with every subject's residues permuted: the device side of the
// statistics calibrated on shuffled subjects (include/cudasw4_amd_shuffle.h).
//
// The unit of work is one dword of output: a thread finds the subject its four bytes belong to, walks the four positions
// through the permutation (four independent cycle walks, issued together so that their multiply chains overlap), gathers
// four bytes of the input and stores one dword.  A workgroup of 256 threads takes 1 KiB of the block, whatever subjects lie
// in it: a 35 000-residue subject is spread over 35 workgroups, fifty 20-residue subjects share one.  blockIdx.y is the
// replica.
//
// Finding the subject: the first and the last subject of the workgroup's KiB are found by two binary searches whose
// arguments depend on blockIdx alone (scalar loads, once per wave); a thread then searches between those two — no step at
// all inside a long subject, about five among 30-residue subjects.
//
// The walk loop is divergent by nature (a lane leaves it when all its four positions have landed below L, after two or
// three passes as a rule); the passes a wave makes are those of its slowest lane.  The gather reads single bytes from
// wherever the permutation points within the subject: a subject of a few KiB stays in the L2 / the vector cache lines the
// neighbouring lanes touch, and the input of a calibration is read once per replica.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace swsh {

constexpr int kThreads = 256;
constexpr int kTileBytes = kThreads * 4;
constexpr int8_t kOther = 20;

__host__ __device__ inline uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}

__host__ __device__ inline uint32_t subject_key(uint32_t seed, int64_t id, uint32_t replica) {
    const uint64_t u = uint64_t(id);
    return mix32(mix32(mix32(mix32(seed) ^ uint32_t(u)) ^ uint32_t(u >> 32)) ^ replica);
}

// h of a true length L >= 2: half the bits of L - 1, rounded up, at least 1
__device__ inline int half_bits(uint32_t L) {
    const int bits = 32 - __clz(int(L - 1));
    const int h = (bits + 1) >> 1;
    return h < 1 ? 1 : h;
}

__device__ inline uint32_t feistel_pass(uint32_t c, uint32_t k, int h, uint32_t mask) {
    uint32_t l = c >> h, r = c & mask;
#pragma unroll
    for (uint32_t rd = 0; rd < 4; rd++) {
        const uint32_t f = mix32(r ^ k ^ (rd * 0x9e3779b9u)) & mask;
        const uint32_t t = l ^ f;
        l = r;
        r = t;
    }
    return (l << h) | r;
}

// the largest i in [lo, hi] with offsets[i] - base <= b (offsets[lo] - base <= b is the caller's)
__device__ inline int32_t last_at_or_below(const uint64_t* __restrict__ offsets, uint64_t base, int32_t lo, int32_t hi, uint64_t b) {
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] - base <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// blockBytes = offsets[n] - offsets[0] (a multiple of 4); grid = (ceil(blockBytes / kTileBytes), replicas of this launch)
__global__ void __launch_bounds__(kThreads) shuffle_subjects_kernel(const int8_t* __restrict__ chars, const uint64_t* __restrict__ offsets,
                                                                    const int32_t* __restrict__ lengths, const int64_t* __restrict__ keys,
                                                                    int32_t n, uint64_t blockBytes, uint32_t seed, uint32_t firstReplica,
                                                                    int8_t* __restrict__ out, uint64_t replicaStride) {
    const uint64_t base = offsets[0];
    const uint64_t tile = uint64_t(blockIdx.x) * kTileBytes;
    const uint64_t tileLast = (tile + kTileBytes <= blockBytes ? tile + kTileBytes : blockBytes) - 4;
    // wave-uniform: the subjects of the tile's first and last dword
    const int32_t sLo = last_at_or_below(offsets, base, 0, n - 1, tile);
    const int32_t sHi = last_at_or_below(offsets, base, sLo, n - 1, tileLast);

    const uint64_t b = tile + uint64_t(threadIdx.x) * 4;
    if (b >= blockBytes) return;
    const int32_t s = last_at_or_below(offsets, base, sLo, sHi, b);
    const uint64_t sBegin = offsets[s] - base;
    const uint64_t sBytes = offsets[s + 1] - base - sBegin;
    int32_t len = lengths[s];
    len = len < 0 ? 0 : len;
    const uint32_t L = uint64_t(len) > sBytes ? uint32_t(sBytes) : uint32_t(len);   // (a gather never leaves the subject)
    const uint32_t p0 = uint32_t(b - sBegin);   // the subject's positions p0 .. p0 + 3

    uint32_t c[4];
    bool real[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        real[j] = p0 + j < L;
        c[j] = real[j] ? p0 + j : 0u;
    }
    if (L >= 2) {
        const uint32_t replica = firstReplica + blockIdx.y;
        const uint32_t k = subject_key(seed, keys ? keys[s] : int64_t(s), replica);
        const int h = half_bits(L);
        const uint32_t mask = (1u << h) - 1u;
        // the first pass of every real position, then all four together for as long as one of them is still outside [0, L)
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (real[j]) c[j] = feistel_pass(c[j], k, h, mask);
        while (c[0] >= L || c[1] >= L || c[2] >= L || c[3] >= L) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t nx = feistel_pass(c[j], k, h, mask);
                c[j] = c[j] >= L ? nx : c[j];
            }
        }
    }
    const int8_t* src = chars + sBegin;
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t byte = real[j] ? uint32_t(uint8_t(src[c[j]])) : uint32_t(uint8_t(kOther));
        word |= byte << (8 * j);
    }
    *reinterpret_cast<uint32_t*>(out + uint64_t(blockIdx.y) * replicaStride + b) = word;
}

}  // namespace swsh
