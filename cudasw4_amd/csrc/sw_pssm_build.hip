// sw_pssm_build.hip — sw_pssm_accumulate (include/cudasw4_amd_pssm.h): the host side of the PSSM-building kernels
// (sw_pssm_build_kernel.hpp).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/cudasw4_amd_pssm.h"
#include "sw_internal.hpp"
#include "sw_pssm_build_kernel.hpp"

namespace {
int hip_fail(hipError_t e, const char* what) {
    return swi::fail(SW_ERR_HIP, std::string("sw_pssm_accumulate: ") + what + ": " + hipGetErrorString(e));
}
}  // namespace

extern "C" int sw_pssm_accumulate(sw_ctx* ctx, const sw_pssm_accumulate_args* a) {
    using swi::fail;
    if (!ctx || !a) return fail(SW_ERR_INVALID, "sw_pssm_accumulate: null argument");
    if (a->qlen < 1 || a->qlen > SW_PSSM_MAX_QUERY_LEN)
        return fail(SW_ERR_INVALID, "sw_pssm_accumulate: qlen must lie in [1, SW_PSSM_MAX_QUERY_LEN]");
    if (a->n < 0) return fail(SW_ERR_INVALID, "sw_pssm_accumulate: n must not be negative");
    if (!a->counts || !a->weights || !a->wcounts || !a->used) return fail(SW_ERR_INVALID, "sw_pssm_accumulate: null output buffer");
    if (a->n > 0 && (!a->chars || !a->offsets || !a->lengths || !a->results || !a->cigar))
        return fail(SW_ERR_INVALID, "sw_pssm_accumulate: null hit buffer");
    if (reinterpret_cast<uintptr_t>(a->counts) % 16 != 0 || reinterpret_cast<uintptr_t>(a->wcounts) % 8 != 0 ||
        reinterpret_cast<uintptr_t>(a->weights) % 8 != 0)
        return fail(SW_ERR_INVALID, "sw_pssm_accumulate: counts must be 16-byte aligned, weights and wcounts 8-byte aligned");
    hipError_t e = hipSetDevice(swi::device_of(ctx));
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    hipStream_t stream = static_cast<hipStream_t>(a->stream);
    auto record = [&](int i) -> hipError_t {
        return a->phase_events ? hipEventRecord(static_cast<hipEvent_t>(a->phase_events[i]), stream) : hipSuccess;
    };
    if ((e = record(0)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    const size_t cells = (size_t)a->qlen * swb::kLetters;
    if ((e = hipMemsetAsync(a->counts, 0, cells * sizeof(uint32_t), stream)) != hipSuccess) return hip_fail(e, "hipMemsetAsync");
    if ((e = hipMemsetAsync(a->wcounts, 0, cells * sizeof(uint64_t), stream)) != hipSuccess) return hip_fail(e, "hipMemsetAsync");
    if ((e = hipMemsetAsync(a->weights, 0, ((size_t)a->n + 1) * sizeof(uint64_t), stream)) != hipSuccess) return hip_fail(e, "hipMemsetAsync");
    if ((e = hipMemsetAsync(a->used, 0, sizeof(int32_t), stream)) != hipSuccess) return hip_fail(e, "hipMemsetAsync");
    swb::BuildParams p{};
    p.query = a->query;
    p.qlen = a->qlen;
    p.n = a->n;
    p.chars = a->chars;
    p.offsets = a->offsets;
    p.lengths = a->lengths;
    p.results = a->results;
    p.cigar = a->cigar;
    p.include = a->include;
    p.counts = a->counts;
    p.weights = reinterpret_cast<unsigned long long*>(a->weights);
    p.wcounts = reinterpret_cast<unsigned long long*>(a->wcounts);
    p.used = a->used;
    const unsigned master_count = a->query ? (unsigned)((a->qlen + swb::kMasterSpan - 1) / swb::kMasterSpan) : 0u;
    const unsigned master_weight = a->query ? 1u : 0u;
    if ((unsigned)a->n + master_count > 0) {
        hipLaunchKernelGGL(swb::pssm_count_kernel, dim3((unsigned)a->n + master_count), dim3(swb::kLanes), 0, stream, p);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "launch (counts)");
        if ((e = record(1)) != hipSuccess) return hip_fail(e, "hipEventRecord");
        hipLaunchKernelGGL(swb::pssm_weight_kernel, dim3((unsigned)a->n + master_weight), dim3(swb::kLanes), 0, stream, p);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "launch (weights)");
    } else if ((e = record(1)) != hipSuccess) {
        return hip_fail(e, "hipEventRecord");
    }
    if ((e = record(2)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    return SW_OK;
}
