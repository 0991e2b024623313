// sw_topk.hip — sw_topk and sw_topk_temp_bytes of the C ABI (include/cudasw4_amd.h).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <string>

#include "../../include/cudasw4_amd.h"
#include "sw_ctx.hpp"

using swi::fail;

extern "C" {

// ------------------------------------------------------------------ top-K
// Replaces the reference's thrust sort_by_key / merge_by_key over ALL scores (cudasw4.cuh:1376-1401).
//   * small inputs, or k >= n: stable descending radix sort of (score, id) pairs, first k copied out;
//   * otherwise a radix SELECT: the composite key (orderable score bits, ~position) is unique, so exactly k
//     elements lie at or above the k-th largest key.  Six histogram passes of 11/11/10 bits (three over the
//     score, three over the position among the ties at the threshold score — skipped on the device when the
//     ties are all taken) find that key reading 4 bytes per element per pass; one more pass compacts the k
//     winners, which are then sorted by their 64-bit keys.  No host round trip: every decision is taken by a
//     one-workgroup kernel that updates a small state block.
// Both paths return the same list: descending score, equal scores in input (position) order — the order the
// driver's position-ordered result lists turn into ascending ids.

namespace {
struct TopkLayout {
    size_t keys_off, vals_off, cub_off, total, cub_bytes;
};
TopkLayout topk_layout(int64_t n) {
    TopkLayout L{};
    size_t cub = 0;
    (void)hipcub::DeviceRadixSort::SortPairsDescending(nullptr, cub, (const float*)nullptr, (float*)nullptr,
                                                       (const int32_t*)nullptr, (int32_t*)nullptr, (int)std::max<int64_t>(n, 1));
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    L.keys_off = 0;
    L.vals_off = al((size_t)n * sizeof(float));
    L.cub_off = L.vals_off + al((size_t)n * sizeof(int32_t));
    L.cub_bytes = cub;
    L.total = L.cub_off + al(cub);
    return L;
}
__global__ void topk_copy_kernel(const float* keys, const int32_t* vals, int64_t n, int k, float* out_s, int32_t* out_i) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < k) {
        out_s[i] = i < n ? keys[i] : -1.0f;
        out_i[i] = i < n ? vals[i] : -1;
    }
}

// ---- radix select
constexpr int kSelBins = 2048;
constexpr int kSelPasses = 6;                      // digits of the 64-bit composite key, most significant first
__constant__ const int kSelShift[kSelPasses] = {53, 42, 32, 21, 10, 0};
__constant__ const int kSelBits[kSelPasses] = {11, 11, 10, 11, 11, 10};

struct TopkState {
    unsigned long long prefix;      // digits of the k-th largest key decided so far (high bits)
    unsigned long long decided;     // mask of the decided bits
    unsigned long long remaining;   // how many elements are still to be taken from the current bucket
    unsigned int skip_rest;         // the whole current bucket is taken: no further passes needed
    unsigned int out_count;         // compaction cursor
    unsigned int blocks_done;       // workgroups of the current histogram pass that have added their part (the last one picks)
    unsigned int hist[kSelBins];
};

__device__ __forceinline__ unsigned long long topk_key(float score, unsigned int pos) {
    unsigned int u = __float_as_uint(score);
    u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;  // monotonic: larger float -> larger unsigned
    return ((unsigned long long)u << 32) | (unsigned long long)(~pos);
}

__global__ void topk_init_kernel(TopkState* st, int k) {
    for (int i = threadIdx.x; i < kSelBins; i += blockDim.x) st->hist[i] = 0;
    if (threadIdx.x == 0) { st->prefix = 0; st->decided = 0; st->remaining = (unsigned long long)k; st->skip_rest = 0; st->out_count = 0; st->blocks_done = 0; }
}

// walk the histogram from the top bin down to the bin that holds the `remaining`-th element (one workgroup of 256 threads;
// h: kSelBins words, part: 256 double words of LDS)
__device__ void topk_pick(TopkState* st, int pass, unsigned int* h, unsigned long long* part) {
    const int nb = 1 << kSelBits[pass];
    for (int i = threadIdx.x; i < kSelBins; i += blockDim.x) { h[i] = i < nb ? __hip_atomic_load(&st->hist[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u; }
    __syncthreads();
    // thread t owns bins [nb - 8(t+1), nb - 8t) (descending): sum, then a serial scan over 256 partial sums by thread 0
    constexpr int per = kSelBins / 256;
    unsigned long long mine = 0;
    for (int j = 0; j < per; j++) { const int b = kSelBins - 1 - (threadIdx.x * per + j); mine += h[b]; }
    part[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long need = st->remaining, above = 0;
        int t = 0;
        while (t < 255 && above + part[t] < need) { above += part[t]; t++; }
        int b = kSelBins - 1 - t * per;
        for (int j = 0; j < per - 1 && above + h[b] < need; j++) { above += h[b]; b--; }
        // bin b holds the element: everything above it is taken
        const int shift = kSelShift[pass];
        st->prefix |= (unsigned long long)b << shift;
        st->decided |= (unsigned long long)((1u << kSelBits[pass]) - 1u) << shift;
        st->remaining = need - above;
        if (st->remaining == h[b]) st->skip_rest = 1;  // the whole bin is taken: its elements need no further ordering
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kSelBins; i += blockDim.x) st->hist[i] = 0;
}

__global__ void __launch_bounds__(256) topk_hist_kernel(const float* __restrict__ scores, int64_t n, TopkState* st, int pass) {
    if (st->skip_rest) return;
    __shared__ unsigned int h[kSelBins];
    for (int i = threadIdx.x; i < kSelBins; i += blockDim.x) h[i] = 0;
    __syncthreads();
    const unsigned long long prefix = st->prefix, decided = st->decided;
    const int shift = kSelShift[pass];
    const unsigned int mask = (1u << kSelBits[pass]) - 1u;
    // The scores of a scan crowd into a few bins of the leading digits (small integers: one exponent), and 64 lanes adding to
    // ONE LDS word serialise — 20 us per pass on 570 000 scores.  So the lanes that share the first active lane's bin add
    // once per wave; the others (the low digits, where few elements are left) add one by one.
    const int wlane = threadIdx.x & 63;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < n; i0 += (int64_t)gridDim.x * blockDim.x) {   // wave-uniform trip count
        const int64_t i = i0 + threadIdx.x;
        bool act = false;
        unsigned int bin = 0;
        if (i < n) {
            const unsigned long long key = topk_key(scores[i], (unsigned int)i);
            act = (key & decided) == prefix;
            bin = (unsigned int)(key >> shift) & mask;
        }
        const unsigned long long m = __ballot(act);
        if (m == 0) continue;
        const unsigned int lb = (unsigned int)__shfl((int)bin, __ffsll((long long)m) - 1);
        const unsigned long long same = __ballot(act && bin == lb);
        if (act) {
            if (bin != lb) atomicAdd(&h[bin], 1u);
            else if (wlane == __ffsll((long long)same) - 1) atomicAdd(&h[lb], (unsigned int)__popcll(same));
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kSelBins; i += blockDim.x)
        if (h[i]) atomicAdd(&st->hist[i], h[i]);
    // the workgroup that adds its part last picks the bin (round 5: was a launch of its own after every pass — twelve small
    // launches per top-K instead of six weigh on a query that is scanned in a millisecond)
    __shared__ unsigned long long part[256];
    __shared__ bool last;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd(&st->blocks_done, 1u) + 1u == gridDim.x;
    __syncthreads();
    if (!last) return;
    __threadfence();
    topk_pick(st, pass, h, part);
    if (threadIdx.x == 0) st->blocks_done = 0;
}

// winners: keys above the decided prefix, or inside it (all of them when skip_rest, else the prefix is a full key)
__global__ void __launch_bounds__(256) topk_compact_kernel(const float* __restrict__ scores, const int32_t* __restrict__ ids, int64_t n,
                                                           TopkState* st, int k, unsigned long long* out_keys, int32_t* out_ids) {
    const unsigned long long prefix = st->prefix, decided = st->decided;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = topk_key(scores[i], (unsigned int)i);
        if ((key & decided) >= prefix) {
            const unsigned int slot = atomicAdd(&st->out_count, 1u);
            if (slot < (unsigned int)k) { out_keys[slot] = key; out_ids[slot] = ids[i]; }
        }
    }
}

__global__ void topk_emit_kernel(const unsigned long long* keys, const int32_t* vals, int k, float* out_s, int32_t* out_i) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < k) {
        unsigned int u = (unsigned int)(keys[i] >> 32);
        u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;
        out_s[i] = __uint_as_float(u);
        out_i[i] = vals[i];
    }
}

// the k winners in descending key order (keys are unique): every element's rank is the number of larger keys — one
// workgroup, k <= 1024 (hipCUB's radix sort of ten 64-bit keys took 15 ... 90 us)
__global__ void __launch_bounds__(256) topk_rank_emit_kernel(const unsigned long long* keys, const int32_t* vals, int k, float* out_s, int32_t* out_i) {
    __shared__ unsigned long long sk[1024];
    for (int i = threadIdx.x; i < k; i += blockDim.x) sk[i] = keys[i];
    __syncthreads();
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        const unsigned long long mine = sk[i];
        int rank = 0;
        for (int j = 0; j < k; j++) rank += sk[j] > mine ? 1 : 0;
        unsigned int u = (unsigned int)(mine >> 32);
        u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;
        out_s[rank] = __uint_as_float(u);
        out_i[rank] = vals[i];
    }
}

// ---- small k (the reference's default: --top 10): two launches instead of nine.  Every workgroup walks chunks of 2 048 scores
// with the k best keys it has seen so far in LDS; a chunk that holds nothing above the k-th best is skipped after one
// block-wide test, otherwise its maxima are extracted one by one (keys are unique: the winner clears its own element).  The
// second kernel does the same over the workgroups' lists and emits the winners in order.  A query that is scanned in a
// millisecond and a half spent 3 % of it in the radix select's nine small launches.
constexpr int kSmallK = 32;
constexpr int kSmallChunk = 2048;   // 256 threads x 8 elements
constexpr int kSmallMaxGrid = 1024;

__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long* wmax) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    __syncthreads();   // (wmax of the round before has been read)
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long m = wmax[0];
#pragma unroll
    for (int w = 1; w < 4; w++) m = wmax[w] > m ? wmax[w] : m;
    return m;
}

// merge the elements key[0..8) of the 256 threads into the descending list best[0..k)
__device__ __forceinline__ void small_merge(unsigned long long (&key)[8], unsigned long long* best, unsigned long long* wmax, int k) {
    unsigned long long mine = 0;
#pragma unroll
    for (int e = 0; e < 8; e++) mine = key[e] > mine ? key[e] : mine;
    for (int round = 0; round < k; round++) {
        // The k-th best is read BEFORE the reduction, not after it: thread 0 inserts m into best[] below, and a wave that
        // came late to a read placed after the reduction could see an m that landed at k-1, take m <= best[k-1] and leave
        // the loop alone.  Here the read follows the insertion of the round before (that round's closing barrier) and
        // precedes this round's (the two barriers inside block_max_u64), so every thread tests the same value.
        const unsigned long long kth = best[k - 1];
        const unsigned long long m = block_max_u64(mine, wmax);
        if (m <= kth) break;           // uniform: nothing of this chunk can still enter
        if (mine == m) {               // unique keys: exactly one thread; it drops the element and finds its next best
            mine = 0;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                if (key[e] == m) key[e] = 0;
                mine = key[e] > mine ? key[e] : mine;
            }
        }
        if (threadIdx.x == 0) {        // sorted insertion
            int i = k - 1;
            while (i > 0 && best[i - 1] < m) { best[i] = best[i - 1]; i--; }
            best[i] = m;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) topk_small_partial_kernel(const float* __restrict__ scores, int64_t n, int k, unsigned long long* out) {
    __shared__ unsigned long long best[kSmallK];
    __shared__ unsigned long long wmax[4];
    if (threadIdx.x < kSmallK) best[threadIdx.x] = 0;
    __syncthreads();
    const int64_t nchunks = (n + kSmallChunk - 1) / kSmallChunk;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        unsigned long long key[8];
        const unsigned long long thr = best[k - 1];
        bool above = false;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int64_t i = c * kSmallChunk + e * 256 + threadIdx.x;
            key[e] = i < n ? topk_key(scores[i], (unsigned int)i) : 0ull;
            above = above || key[e] > thr;
        }
        if (!__syncthreads_or(above)) continue;
        small_merge(key, best, wmax, k);
    }
    __syncthreads();
    if (threadIdx.x < k) out[(size_t)blockIdx.x * k + threadIdx.x] = best[threadIdx.x];
}

__global__ void __launch_bounds__(256) topk_small_final_kernel(const unsigned long long* __restrict__ cand, int ncand, const int32_t* __restrict__ ids,
                                                               int k, float* out_s, int32_t* out_i) {
    __shared__ unsigned long long best[kSmallK];
    __shared__ unsigned long long wmax[4];
    if (threadIdx.x < kSmallK) best[threadIdx.x] = 0;
    __syncthreads();
    for (int c0 = 0; c0 < ncand; c0 += kSmallChunk) {
        unsigned long long key[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int i = c0 + e * 256 + threadIdx.x;
            key[e] = i < ncand ? cand[i] : 0ull;
        }
        small_merge(key, best, wmax, k);
    }
    __syncthreads();
    if (threadIdx.x < k) {
        const unsigned long long key = best[threadIdx.x];
        unsigned int u = (unsigned int)(key >> 32);
        u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;
        out_s[threadIdx.x] = __uint_as_float(u);
        out_i[threadIdx.x] = ids[~(unsigned int)key];
    }
}

int small_grid(const sw_ctx* ctx, int64_t n) {
    const int64_t nchunks = (n + kSmallChunk - 1) / kSmallChunk;
    return (int)std::max<int64_t>(1, std::min<int64_t>(nchunks, std::min<int64_t>(kSmallMaxGrid, (int64_t)std::max(1, ctx->plan.num_cus) * 4)));
}

struct SelectLayout {
    size_t state_off, keys_a, keys_b, vals_a, vals_b, cub_off, cub_bytes, total;
};
SelectLayout select_layout(int k) {
    SelectLayout L{};
    size_t cub = 0;
    (void)hipcub::DeviceRadixSort::SortPairsDescending(nullptr, cub, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                                       (const int32_t*)nullptr, (int32_t*)nullptr, std::max(k, 1));
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    L.state_off = 0;
    L.keys_a = al(sizeof(TopkState));
    L.keys_b = L.keys_a + al((size_t)k * 8);
    L.vals_a = L.keys_b + al((size_t)k * 8);
    L.vals_b = L.vals_a + al((size_t)k * 4);
    L.cub_off = L.vals_b + al((size_t)k * 4);
    L.cub_bytes = cub;
    L.total = L.cub_off + al(cub);
    return L;
}

// the select pays off once the sort's passes over all n pairs dominate; CUDASW4_AMD_TOPK=sort|select forces a path (tests)
bool use_select(int64_t n, int k) {
    const char* force = getenv("CUDASW4_AMD_TOPK");
    if (k >= n) return false;
    if (force && force[0] == 's' && force[1] == 'o') return false;
    if (force && force[0] == 's' && force[1] == 'e') return true;
    return n >= (int64_t(1) << 17) && (int64_t)k * 8 <= n;
}
}  // namespace

size_t sw_topk_temp_bytes(int64_t n, int k) {
    if (n <= 0 || k <= 0) return 0;
    // sized for any path, so that a forced path (tests) never outgrows a buffer sized by this call
    return std::max(std::max(topk_layout(n).total, k < n ? select_layout(k).total : size_t(0)), (size_t)kSmallMaxGrid * kSmallK * sizeof(unsigned long long));
}

int sw_topk(sw_ctx* ctx, const float* scores, const int32_t* ids, int64_t n, int k, float* out_scores,
            int32_t* out_ids, void* temp, size_t temp_bytes, void* stream) {
    if (!ctx) return fail(SW_ERR_INVALID, "null context");
    if (k <= 0) return SW_OK;
    if (n < 0 || n > 0x7fffffffLL) return fail(SW_ERR_INVALID, "bad result count");
    if (!out_scores || !out_ids) return fail(SW_ERR_INVALID, "null output");
    SW_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n > 0 && (!scores || !ids)) return fail(SW_ERR_INVALID, "null input");
    const char* force = getenv("CUDASW4_AMD_TOPK");
    if (n > k && k <= kSmallK && (!force || (force[0] == 's' && force[1] == 'm'))) {   // CUDASW4_AMD_TOPK=small|select|sort forces a path (tests)
        const int grid = small_grid(ctx, n);
        if (!temp || temp_bytes < (size_t)grid * k * sizeof(unsigned long long)) return fail(SW_ERR_TEMP, "temp buffer too small for top-K");
        unsigned long long* cand = static_cast<unsigned long long*>(temp);
        hipLaunchKernelGGL(topk_small_partial_kernel, dim3(grid), dim3(256), 0, s, scores, n, k, cand);
        hipLaunchKernelGGL(topk_small_final_kernel, dim3(1), dim3(256), 0, s, cand, grid * k, ids, k, out_scores, out_ids);
        SW_HIP(hipGetLastError());
        return SW_OK;
    }
    if (n > 0 && use_select(n, k)) {
        const SelectLayout L = select_layout(k);
        if (!temp || temp_bytes < L.total) return fail(SW_ERR_TEMP, "temp buffer too small for top-K");
        char* base = static_cast<char*>(temp);
        TopkState* st = reinterpret_cast<TopkState*>(base + L.state_off);
        auto* keys_a = reinterpret_cast<unsigned long long*>(base + L.keys_a);
        auto* keys_b = reinterpret_cast<unsigned long long*>(base + L.keys_b);
        auto* vals_a = reinterpret_cast<int32_t*>(base + L.vals_a);
        auto* vals_b = reinterpret_cast<int32_t*>(base + L.vals_b);
        const int grid = (int)std::min<int64_t>((n + 256 * 16 - 1) / (256 * 16), (int64_t)std::max(1, ctx->plan.num_cus) * 8);
        hipLaunchKernelGGL(topk_init_kernel, dim3(1), dim3(256), 0, s, st, k);
        for (int pass = 0; pass < kSelPasses; pass++) {
            hipLaunchKernelGGL(topk_hist_kernel, dim3(grid), dim3(256), 0, s, scores, n, st, pass);
        }
        hipLaunchKernelGGL(topk_compact_kernel, dim3(grid), dim3(256), 0, s, scores, ids, n, st, k, keys_a, vals_a);
        SW_HIP(hipGetLastError());
        if (k <= 1024) {
            hipLaunchKernelGGL(topk_rank_emit_kernel, dim3(1), dim3(256), 0, s, keys_a, vals_a, k, out_scores, out_ids);
        } else {
            size_t cub = L.cub_bytes;
            SW_HIP(hipcub::DeviceRadixSort::SortPairsDescending(base + L.cub_off, cub, keys_a, keys_b, vals_a, vals_b, k, 0, 64, s));
            hipLaunchKernelGGL(topk_emit_kernel, dim3((k + 255) / 256), dim3(256), 0, s, keys_b, vals_b, k, out_scores, out_ids);
        }
        SW_HIP(hipGetLastError());
        return SW_OK;
    }
    float* keys = nullptr;
    int32_t* vals = nullptr;
    if (n > 0) {
        const TopkLayout L = topk_layout(n);
        if (!temp || temp_bytes < L.total) return fail(SW_ERR_TEMP, "temp buffer too small for top-K");
        char* base = static_cast<char*>(temp);
        keys = reinterpret_cast<float*>(base + L.keys_off);
        vals = reinterpret_cast<int32_t*>(base + L.vals_off);
        size_t cub = L.cub_bytes;
        SW_HIP(hipcub::DeviceRadixSort::SortPairsDescending(base + L.cub_off, cub, scores, keys, ids, vals, (int)n, 0, 32, s));
    }
    hipLaunchKernelGGL(topk_copy_kernel, dim3((k + 255) / 256), dim3(256), 0, s, keys, vals, n, k, out_scores, out_ids);
    SW_HIP(hipGetLastError());
    return SW_OK;
}

}  // extern "C"
