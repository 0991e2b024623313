// sw_stats_kernel.hpp — the (length bin, score) histogram of a scan's scores: the device side of the search statistics
// (include/cudasw4_amd_stats.h).
//
// A persistent grid of 256-thread workgroups, each with the whole table as one 64 KiB LDS tile (two workgroups fit a CU's
// 160 KiB).  A lane loads four subjects at a time (16 bytes of scores, 16 of lengths), adds them to the tile with integer
// LDS atomics, and at the end the workgroup adds the non-zero words of its tile to the table in memory.
//
// The hazard is the one topk_hist_kernel (sw_topk.hip) met: a DB is sorted by length and the scores of unrelated subjects
// crowd into about 20 values, so the lanes of a wave hit a handful of LDS words, and 64 lanes adding to ONE word
// serialise.  The remedy is the same: the lanes that share the first active lane's word add once, with their count.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sws {

constexpr int kLBins = 64, kSBins = 256, kThreads = 256;
// subjects a workgroup should at least have (below that the grid shrinks: zeroing and flushing a 64 KiB tile, and the
// atomics of the flush, are what a small launch costs)
constexpr int64_t kMinPerGroup = 4096;

__host__ __device__ inline int length_bin(int32_t L) {
    if (L <= 1) return 0;
#ifdef __HIP_DEVICE_COMPILE__
    const int e = 31 - __clz(L);
#else
    const int e = 31 - __builtin_clz((unsigned)L);
#endif
    return 2 * e + ((L >> (e - 1)) & 1);
}

// The n subjects are cut into an unaligned head (`head` <= 3 subjects, up to the first 16-byte boundary of `scores`), a
// middle of `nvec` groups of four, and a tail (<= 3): 0 <= head, head + 4 nvec <= n < head + 4 nvec + 4.
// kVecLengths: the lengths of the middle are 16-byte aligned as well (the usual case: both arrays of a scan start aligned
// and are offset alike); otherwise they are loaded one by one
template <bool kVecLengths>
__global__ void __launch_bounds__(kThreads) score_hist_kernel(const float* __restrict__ scores, const int32_t* __restrict__ lengths,
                                                              int64_t n, int64_t head, int64_t nvec, unsigned int* __restrict__ hist,
                                                              unsigned long long* __restrict__ sumlen, unsigned int* __restrict__ skipped) {
    __shared__ __attribute__((aligned(16))) unsigned int tile[kLBins * kSBins];
    __shared__ unsigned long long lenSum[kLBins];
    __shared__ unsigned int skippedSum;
    {
        uint4* t4 = reinterpret_cast<uint4*>(tile);
        for (int i = threadIdx.x; i < kLBins * kSBins / 4; i += kThreads) t4[i] = make_uint4(0, 0, 0, 0);
        if (threadIdx.x < kLBins) lenSum[threadIdx.x] = 0;
        if (threadIdx.x == 0) skippedSum = 0;
    }
    __syncthreads();

    const int wlane = threadIdx.x & 63;
    // a thread's subjects ascend, and so do their lengths in a sorted DB: the lengths are summed in a register and added to
    // the bin's LDS word when the bin changes
    int curBin = 0;
    unsigned long long curLen = 0;
    unsigned int nskip = 0;
    auto add = [&](bool present, float score, int32_t L) {
        const bool binned = present && score >= 0.0f;   // (NaN: skipped)
        if (present && !binned) nskip++;
        unsigned int word = 0;
        if (binned) {
            const int lb = length_bin(L);
            const int sb = score >= float(kSBins - 1) ? kSBins - 1 : int(score);
            word = (unsigned int)(lb * kSBins + sb);
            if (lb != curBin) {
                if (curLen) atomicAdd(&lenSum[curBin], curLen);
                curBin = lb;
                curLen = 0;
            }
            curLen += (unsigned long long)(L > 0 ? L : 0);
        }
        const unsigned long long m = __ballot(binned);
        if (m == 0) return;
        const int lead = __ffsll((long long)m) - 1;
        const unsigned int lw = (unsigned int)__shfl((int)word, lead);
        const unsigned long long same = __ballot(binned && word == lw);
        if (binned) {
            if (word != lw) atomicAdd(&tile[word], 1u);
            else if (wlane == lead) atomicAdd(&tile[lw], (unsigned int)__popcll(same));
        }
    };

    // the unaligned head and tail (at most three subjects each): the first wave of the first workgroup
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        const int64_t tailBegin = head + 4 * nvec;
        const bool h = wlane < head, t = tailBegin + wlane < n;
        add(h, h ? scores[wlane] : 0.0f, h ? lengths[wlane] : 0);
        add(t, t ? scores[tailBegin + wlane] : 0.0f, t ? lengths[tailBegin + wlane] : 0);
    }
    const float4* s4 = reinterpret_cast<const float4*>(scores + head);
    const int32_t* lmid = lengths + head;
    for (int64_t v0 = (int64_t)blockIdx.x * kThreads; v0 < nvec; v0 += (int64_t)gridDim.x * kThreads) {   // wave-uniform trip count
        const int64_t v = v0 + threadIdx.x;
        const bool present = v < nvec;
        float4 s = make_float4(0, 0, 0, 0);
        int4 l = make_int4(0, 0, 0, 0);
        if (present) {
            s = s4[v];
            if (kVecLengths) l = reinterpret_cast<const int4*>(lmid)[v];
            else l = make_int4(lmid[4 * v], lmid[4 * v + 1], lmid[4 * v + 2], lmid[4 * v + 3]);
        }
        add(present, s.x, l.x);
        add(present, s.y, l.y);
        add(present, s.z, l.z);
        add(present, s.w, l.w);
    }

    // what the registers still hold: reduced over the wave where its lanes agree on the bin, one LDS add per wave
    {
        const bool have = curLen != 0;
        const unsigned long long m = __ballot(have);
        if (m) {
            const int lead = __ffsll((long long)m) - 1;
            const int lb = __shfl(curBin, lead);
            const bool mine = have && curBin == lb;
            unsigned long long sum = mine ? curLen : 0;
            for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
            if (wlane == lead) atomicAdd(&lenSum[lb], sum);
            else if (have && !mine) atomicAdd(&lenSum[curBin], curLen);
        }
        unsigned int sk = nskip;
        for (int d = 32; d >= 1; d >>= 1) sk += (unsigned int)__shfl_xor((int)sk, d);
        if (wlane == 0 && sk) atomicAdd(&skippedSum, sk);
    }
    __syncthreads();

    // flush: the non-zero words only (a sorted DB's workgroup touches a few length bins and a few dozen scores)
    {
        const uint4* t4 = reinterpret_cast<const uint4*>(tile);
        for (int i = threadIdx.x; i < kLBins * kSBins / 4; i += kThreads) {
            const uint4 w = t4[i];
            if ((w.x | w.y | w.z | w.w) == 0) continue;
            if (w.x) atomicAdd(&hist[4 * i], w.x);
            if (w.y) atomicAdd(&hist[4 * i + 1], w.y);
            if (w.z) atomicAdd(&hist[4 * i + 2], w.z);
            if (w.w) atomicAdd(&hist[4 * i + 3], w.w);
        }
        if (threadIdx.x < kLBins && lenSum[threadIdx.x]) atomicAdd(&sumlen[threadIdx.x], lenSum[threadIdx.x]);
        if (threadIdx.x == 0 && skippedSum) atomicAdd(skipped, skippedSum);
    }
}

}  // namespace sws
