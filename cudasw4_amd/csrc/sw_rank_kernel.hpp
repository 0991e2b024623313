// sw_rank_kernel.hpp — Z-score keys of a scan's scores, and the gather behind the top-K over them: the device side of the
// ranking by E-value (include/cudasw4_amd_rank.h).
//
// zscore_keys_kernel streams 12 bytes per subject (score and length in, key out; 16 with the positions): 256-thread
// workgroups in a grid-stride loop, four subjects per lane and step with 16-byte accesses wherever an array's middle is
// 16-byte aligned.  The logarithm and the comparison with the threshold are double precision (the key is the ROUNDED z; the
// count is taken before the rounding).  The count goes ballot -> popcount per wave (a wave-uniform sum), one LDS add per
// wave, one atomic per workgroup.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace swr {

constexpr int kThreads = 256;
constexpr float kKeyNone = -3.0e38f, kKeyLimit = 2.9e38f;
// which of the arrays' middles (from the first 16-byte boundary of `scores` on) are 16-byte aligned as well
constexpr unsigned kVecLengths = 1, kVecKeys = 2, kVecPositions = 4;

// The n subjects are cut like score_hist_kernel's (sw_stats_kernel.hpp): an unaligned head (`head` <= 3 subjects, up to the
// first 16-byte boundary of `scores`), a middle of `nvec` groups of four, and a tail (<= 3):
// 0 <= head, head + 4 nvec <= n < head + 4 nvec + 4.
__global__ void __launch_bounds__(kThreads) zscore_keys_kernel(const float* __restrict__ scores, const int32_t* __restrict__ lengths,
                                                               int64_t n, int64_t head, int64_t nvec, double a, double b1, double sd,
                                                               double zmin, float* __restrict__ keys, int32_t* __restrict__ positions,
                                                               unsigned long long* __restrict__ count, unsigned vec) {
    __shared__ unsigned long long groupCount;
    if (threadIdx.x == 0) groupCount = 0;
    __syncthreads();

    const int wlane = threadIdx.x & 63;
    unsigned long long waveCount = 0;   // wave-uniform: every call of key_of is in wave-uniform control flow
    auto key_of = [&](bool present, float score, int32_t L) -> float {
        float key = kKeyNone;
        bool counted = false;
        if (present && score >= 0.0f) {   // (NaN: not scored)
            const double z = (double(score) - a - b1 * log(double(L < 1 ? 1 : L))) / sd;
            counted = z >= zmin;
            key = fminf(fmaxf(float(z), -kKeyLimit), kKeyLimit);
        }
        waveCount += (unsigned long long)__popcll(__ballot(counted));
        return key;
    };

    // the unaligned head and tail (at most three subjects each): the first wave of the first workgroup
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        const int64_t tailBegin = head + 4 * nvec;
        const bool h = wlane < head, t = tailBegin + wlane < n;
        const float kh = key_of(h, h ? scores[wlane] : 0.0f, h ? lengths[wlane] : 0);
        const float kt = key_of(t, t ? scores[tailBegin + wlane] : 0.0f, t ? lengths[tailBegin + wlane] : 0);
        if (h) {
            keys[wlane] = kh;
            if (positions) positions[wlane] = wlane;
        }
        if (t) {
            keys[tailBegin + wlane] = kt;
            if (positions) positions[tailBegin + wlane] = int32_t(tailBegin + wlane);
        }
    }
    const float4* s4 = reinterpret_cast<const float4*>(scores + head);
    const int32_t* lmid = lengths + head;
    float* kmid = keys + head;
    for (int64_t v0 = (int64_t)blockIdx.x * kThreads; v0 < nvec; v0 += (int64_t)gridDim.x * kThreads) {   // wave-uniform trip count
        const int64_t v = v0 + threadIdx.x;
        const bool present = v < nvec;
        float4 s = make_float4(0, 0, 0, 0);
        int4 l = make_int4(0, 0, 0, 0);
        if (present) {
            s = s4[v];
            if (vec & kVecLengths) l = reinterpret_cast<const int4*>(lmid)[v];
            else l = make_int4(lmid[4 * v], lmid[4 * v + 1], lmid[4 * v + 2], lmid[4 * v + 3]);
        }
        float4 k;
        k.x = key_of(present, s.x, l.x);
        k.y = key_of(present, s.y, l.y);
        k.z = key_of(present, s.z, l.z);
        k.w = key_of(present, s.w, l.w);
        if (present && (vec & kVecKeys)) {
            reinterpret_cast<float4*>(kmid)[v] = k;
        } else if (present) {
            kmid[4 * v] = k.x; kmid[4 * v + 1] = k.y; kmid[4 * v + 2] = k.z; kmid[4 * v + 3] = k.w;
        }
        if (present && positions) {
            const int32_t p = int32_t(head + 4 * v);   // n < 2^31
            int32_t* pmid = positions + head;
            if (vec & kVecPositions) {
                reinterpret_cast<int4*>(pmid)[v] = make_int4(p, p + 1, p + 2, p + 3);
            } else {
                pmid[4 * v] = p; pmid[4 * v + 1] = p + 1; pmid[4 * v + 2] = p + 2; pmid[4 * v + 3] = p + 3;
            }
        }
    }

    if (wlane == 0 && waveCount) atomicAdd(&groupCount, waveCount);
    __syncthreads();
    if (threadIdx.x == 0 && groupCount) atomicAdd(count, groupCount);
}

// one thread per chosen position
__global__ void __launch_bounds__(kThreads) gather_hits_kernel(const int32_t* __restrict__ positions, int k, const float* __restrict__ scores,
                                                               const int32_t* __restrict__ ids, float* __restrict__ out_scores,
                                                               int32_t* __restrict__ out_ids) {
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= k) return;
    const int32_t p = positions[j];
    out_scores[j] = p >= 0 ? scores[p] : -1.0f;
    out_ids[j] = p >= 0 ? ids[p] : -1;
}

}  // namespace swr
