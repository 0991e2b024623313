// sw_stats.hip — sw_score_histogram (include/cudasw4_amd_stats.h): the host side of the histogram kernel
// (sw_stats_kernel.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/cudasw4_amd_stats.h"
#include "sw_internal.hpp"
#include "sw_stats_kernel.hpp"

static_assert(sws::kLBins == SW_STATS_LBINS && sws::kSBins == SW_STATS_SBINS, "the kernel's tile is the header's table");

extern "C" int sw_score_histogram(sw_ctx* ctx, const float* scores, const int32_t* lengths, int64_t n, uint32_t* hist,
                                  uint64_t* sumlen, uint32_t* skipped, void* stream) {
    using swi::fail;
    if (!ctx) return fail(SW_ERR_INVALID, "sw_score_histogram: null context");
    if (n < 0) return fail(SW_ERR_INVALID, "sw_score_histogram: n must not be negative");
    if (n == 0) return SW_OK;
    if (!scores || !lengths || !hist || !sumlen || !skipped) return fail(SW_ERR_INVALID, "sw_score_histogram: null pointer");
    if (reinterpret_cast<uintptr_t>(scores) % 4 != 0 || reinterpret_cast<uintptr_t>(lengths) % 4 != 0 ||
        reinterpret_cast<uintptr_t>(hist) % 4 != 0 || reinterpret_cast<uintptr_t>(sumlen) % 8 != 0 ||
        reinterpret_cast<uintptr_t>(skipped) % 4 != 0)
        return fail(SW_ERR_INVALID, "sw_score_histogram: scores, lengths, hist and skipped must be 4-byte aligned, sumlen 8-byte aligned");
    hipError_t e = hipSetDevice(swi::device_of(ctx));
    if (e != hipSuccess) return fail(SW_ERR_HIP, std::string("sw_score_histogram: hipSetDevice: ") + hipGetErrorString(e));
    // subjects up to the first 16-byte boundary of the scores, then groups of four
    const int64_t head = std::min<int64_t>(n, int64_t((16 - reinterpret_cast<uintptr_t>(scores) % 16) % 16 / 4));
    const int64_t nvec = (n - head) / 4;
    const bool vecLengths = reinterpret_cast<uintptr_t>(lengths + head) % 16 == 0;
    const int64_t want = (n + sws::kMinPerGroup - 1) / sws::kMinPerGroup;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, 2 * (int64_t)std::max(swi::num_cus(ctx), 1)));
    auto* h = reinterpret_cast<unsigned int*>(hist);
    auto* sl = reinterpret_cast<unsigned long long*>(sumlen);
    auto* sk = reinterpret_cast<unsigned int*>(skipped);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vecLengths) hipLaunchKernelGGL(sws::score_hist_kernel<true>, dim3(grid), dim3(sws::kThreads), 0, s, scores, lengths, n, head, nvec, h, sl, sk);
    else hipLaunchKernelGGL(sws::score_hist_kernel<false>, dim3(grid), dim3(sws::kThreads), 0, s, scores, lengths, n, head, nvec, h, sl, sk);
    if ((e = hipGetLastError()) != hipSuccess) return fail(SW_ERR_HIP, std::string("sw_score_histogram: launch: ") + hipGetErrorString(e));
    return SW_OK;
}
