// sw_rank.hip — sw_zscore_keys and sw_gather_hits (include/cudasw4_amd_rank.h): the host side of the kernels of
// sw_rank_kernel.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/cudasw4_amd_rank.h"
#include "sw_internal.hpp"
#include "sw_rank_kernel.hpp"

static_assert(swr::kKeyNone == SW_RANK_KEY_NONE && swr::kKeyLimit == SW_RANK_KEY_LIMIT, "the kernel's constants are the header's");

namespace {
bool aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }
}  // namespace

extern "C" int sw_zscore_keys(sw_ctx* ctx, const float* scores, const int32_t* lengths, int64_t n, double a, double b1, double sd,
                              double z_min, float* keys, int32_t* positions, unsigned long long* count, void* stream) {
    using swi::fail;
    if (!ctx) return fail(SW_ERR_INVALID, "sw_zscore_keys: null context");
    if (!std::isfinite(a) || !std::isfinite(b1) || !std::isfinite(sd) || !std::isfinite(z_min))
        return fail(SW_ERR_INVALID, "sw_zscore_keys: a, b1, sd and z_min must be finite (no threshold: z_min = -DBL_MAX)");
    if (!(sd > 0.0)) return fail(SW_ERR_INVALID, "sw_zscore_keys: sd must be positive");
    if (n < 0 || n >= (int64_t(1) << 31)) return fail(SW_ERR_INVALID, "sw_zscore_keys: n must be in [0, 2^31)");
    if (n == 0) return SW_OK;
    if (!scores || !lengths || !keys || !count) return fail(SW_ERR_INVALID, "sw_zscore_keys: null pointer");
    if (!aligned(scores, 4) || !aligned(lengths, 4) || !aligned(keys, 4) || !aligned(positions, 4) || !aligned(count, 8))
        return fail(SW_ERR_INVALID, "sw_zscore_keys: scores, lengths, keys and positions must be 4-byte aligned, count 8-byte aligned");
    hipError_t e = hipSetDevice(swi::device_of(ctx));
    if (e != hipSuccess) return fail(SW_ERR_HIP, std::string("sw_zscore_keys: hipSetDevice: ") + hipGetErrorString(e));
    // subjects up to the first 16-byte boundary of the scores, then groups of four
    const int64_t head = std::min<int64_t>(n, int64_t((16 - reinterpret_cast<uintptr_t>(scores) % 16) % 16 / 4));
    const int64_t nvec = (n - head) / 4;
    unsigned vec = 0;
    if (aligned(lengths + head, 16)) vec |= swr::kVecLengths;
    if (aligned(keys + head, 16)) vec |= swr::kVecKeys;
    if (positions && aligned(positions + head, 16)) vec |= swr::kVecPositions;
    const int64_t want = (nvec + swr::kThreads - 1) / swr::kThreads;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, 8 * (int64_t)std::max(swi::num_cus(ctx), 1)));
    hipLaunchKernelGGL(swr::zscore_keys_kernel, dim3(grid), dim3(swr::kThreads), 0, static_cast<hipStream_t>(stream), scores, lengths, n,
                       head, nvec, a, b1, sd, z_min, keys, positions, count, vec);
    if ((e = hipGetLastError()) != hipSuccess) return fail(SW_ERR_HIP, std::string("sw_zscore_keys: launch: ") + hipGetErrorString(e));
    return SW_OK;
}

extern "C" int sw_gather_hits(sw_ctx* ctx, const int32_t* positions, int k, const float* scores, const int32_t* ids, float* out_scores,
                              int32_t* out_ids, void* stream) {
    using swi::fail;
    if (!ctx) return fail(SW_ERR_INVALID, "sw_gather_hits: null context");
    if (k < 0) return fail(SW_ERR_INVALID, "sw_gather_hits: k must not be negative");
    if (k == 0) return SW_OK;
    if (!positions || !scores || !ids || !out_scores || !out_ids) return fail(SW_ERR_INVALID, "sw_gather_hits: null pointer");
    hipError_t e = hipSetDevice(swi::device_of(ctx));
    if (e != hipSuccess) return fail(SW_ERR_HIP, std::string("sw_gather_hits: hipSetDevice: ") + hipGetErrorString(e));
    hipLaunchKernelGGL(swr::gather_hits_kernel, dim3((unsigned)((k + swr::kThreads - 1) / swr::kThreads)), dim3(swr::kThreads), 0,
                       static_cast<hipStream_t>(stream), positions, k, scores, ids, out_scores, out_ids);
    if ((e = hipGetLastError()) != hipSuccess) return fail(SW_ERR_HIP, std::string("sw_gather_hits: launch: ") + hipGetErrorString(e));
    return SW_OK;
}
