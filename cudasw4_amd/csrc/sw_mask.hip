// sw_mask.hip — sw_mask_subjects (include/cudasw4_amd_mask.h): the host side of the masking kernels (sw_mask_kernel.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/cudasw4_amd_mask.h"
#include "sw_internal.hpp"
#include "sw_mask_kernel.hpp"

namespace {
size_t scratch_for(uint64_t bytes) { return size_t(3 * swmk::words_of(bytes) * sizeof(uint64_t)); }
}  // namespace

// phases: nullptr, or four events recorded around the three launches (one range only)
static int mask_subjects(sw_ctx* ctx, const int8_t* chars, const uint64_t* offsets, const int32_t* lengths, int32_t n,
                         const sw_mask_params* p, int8_t* out, void* temp, size_t temp_bytes, size_t* temp_bytes_needed,
                         unsigned long long* counts, void* stream, void* const* phases) {
    using swi::fail;
    if (!ctx) return fail(SW_ERR_INVALID, "sw_mask_subjects: null context");
    if (n < 0) return fail(SW_ERR_INVALID, "sw_mask_subjects: n must not be negative");
    if (!p) return fail(SW_ERR_INVALID, "sw_mask_subjects: null parameters");
    if (p->window < SW_MASK_MIN_WINDOW || p->window > SW_MASK_MAX_WINDOW) return fail(SW_ERR_INVALID, "sw_mask_subjects: the window must be 4 .. 32");
    if (p->extend_sum < 1 || p->trigger_sum < p->extend_sum) return fail(SW_ERR_INVALID, "sw_mask_subjects: 1 <= extend_sum <= trigger_sum is required");
    if (!temp && !temp_bytes_needed) return fail(SW_ERR_INVALID, "sw_mask_subjects: neither scratch nor a place for its size");
    if (n == 0) {
        if (temp_bytes_needed) *temp_bytes_needed = 0;
        return SW_OK;
    }
    if (!offsets) return fail(SW_ERR_INVALID, "sw_mask_subjects: null pointer");
    if (reinterpret_cast<uintptr_t>(offsets) % 8 != 0) return fail(SW_ERR_INVALID, "sw_mask_subjects: offsets must be 8-byte aligned");
    hipError_t e = hipSetDevice(swi::device_of(ctx));
    if (e != hipSuccess) return fail(SW_ERR_HIP, std::string("sw_mask_subjects: hipSetDevice: ") + hipGetErrorString(e));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the two ends of the block: its size decides the scratch and the grids
    uint64_t ends[2] = {0, 0};
    if ((e = hipMemcpyAsync(&ends[0], offsets, sizeof(uint64_t), hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipMemcpyAsync(&ends[1], offsets + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
        return fail(SW_ERR_HIP, std::string("sw_mask_subjects: reading the block's ends: ") + hipGetErrorString(e));
    if (ends[1] < ends[0] || (ends[1] - ends[0]) % 4 != 0)
        return fail(SW_ERR_INVALID, "sw_mask_subjects: offsets must ascend and the block must be a multiple of 4 bytes");
    const uint64_t blockBytes = ends[1] - ends[0];
    const size_t needAll = scratch_for(blockBytes);
    if (temp_bytes_needed) *temp_bytes_needed = needAll;
    if (!temp) return SW_OK;
    if (!chars || !lengths || !out) return fail(SW_ERR_INVALID, "sw_mask_subjects: null pointer");
    if (reinterpret_cast<uintptr_t>(chars) % 4 != 0 || reinterpret_cast<uintptr_t>(out) % 4 != 0 || reinterpret_cast<uintptr_t>(lengths) % 4 != 0 ||
        reinterpret_cast<uintptr_t>(temp) % 8 != 0 || reinterpret_cast<uintptr_t>(counts) % 8 != 0)
        return fail(SW_ERR_INVALID, "sw_mask_subjects: chars, out and lengths must be 4-byte aligned, temp and counts 8-byte aligned");
    if (out != chars && out < chars + blockBytes && chars < out + blockBytes)
        return fail(SW_ERR_INVALID, "sw_mask_subjects: out must be chars or must not overlap the block");
    if (blockBytes == 0) return SW_OK;

    // ranges of whole subjects whose bitmaps fit the scratch: one when it holds the block, else by the offsets
    std::vector<swmk::Range> ranges;
    if (temp_bytes >= needAll) {
        ranges.push_back(swmk::Range{0, blockBytes, 0, n});
    } else {
        std::vector<uint64_t> off(size_t(n) + 1);
        if ((e = hipMemcpyAsync(off.data(), offsets, off.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s)) != hipSuccess ||
            (e = hipStreamSynchronize(s)) != hipSuccess)
            return fail(SW_ERR_HIP, std::string("sw_mask_subjects: reading the offsets: ") + hipGetErrorString(e));
        uint64_t longest = 0;
        for (int32_t i = 0; i < n; i++) {
            if (off[size_t(i) + 1] < off[size_t(i)] || (off[size_t(i) + 1] - off[size_t(i)]) % 4 != 0)
                return fail(SW_ERR_INVALID, "sw_mask_subjects: offsets must ascend in steps of multiples of 4 bytes");
            longest = std::max(longest, off[size_t(i) + 1] - off[size_t(i)]);
        }
        if (scratch_for(longest) > temp_bytes)
            return fail(SW_ERR_INVALID, "sw_mask_subjects: the scratch cannot hold the longest subject: " + std::to_string(scratch_for(longest)) +
                                            " bytes are needed for it, " + std::to_string(needAll) + " for the whole block, " +
                                            std::to_string(temp_bytes) + " were given");
        for (int32_t first = 0; first < n;) {
            int32_t last = first + 1;   // exclusive
            while (last < n && scratch_for(off[size_t(last) + 1] - off[size_t(first)]) <= temp_bytes) last++;
            ranges.push_back(swmk::Range{off[size_t(first)] - off[0], off[size_t(last)] - off[size_t(first)], first, last - first});
            first = last;
        }
    }

    if (phases && ranges.size() != 1) return fail(SW_ERR_INVALID, "sw_mask_subjects_phases: the scratch must take the block in one go");
    auto mark = [&](int i) { return phases ? hipEventRecord(static_cast<hipEvent_t>(phases[i]), s) : hipSuccess; };
    for (const swmk::Range& r : ranges) {
        if (r.bytes == 0) continue;
        const uint64_t words = swmk::words_of(r.bytes);
        uint64_t* lo = static_cast<uint64_t*>(temp);
        uint64_t* trig = lo + words;
        uint64_t* keep = trig + words;
        const uint64_t tiles = (r.bytes + swmk::kTileBytes - 1) / swmk::kTileBytes;
        const uint64_t applyTiles = (r.bytes + swmk::kApplyTileBytes - 1) / swmk::kApplyTileBytes;
        if (applyTiles > 0x7fffffffull) return fail(SW_ERR_INVALID, "sw_mask_subjects: the block is too large for one call");
        (void)mark(0);
        hipLaunchKernelGGL(swmk::flags_kernel, dim3(unsigned(tiles)), dim3(swmk::kThreads), 0, s, chars, offsets, lengths, r, p->window,
                           p->trigger_sum, p->extend_sum, lo, trig, keep);
        if ((e = hipGetLastError()) != hipSuccess) return fail(SW_ERR_HIP, std::string("sw_mask_subjects: launch (flags): ") + hipGetErrorString(e));
        (void)mark(1);
        hipLaunchKernelGGL(swmk::resolve_kernel, dim3(unsigned((r.count + swmk::kThreads - 1) / swmk::kThreads)), dim3(swmk::kThreads), 0, s,
                           offsets, lengths, r, p->window, lo, trig, keep, counts);
        if ((e = hipGetLastError()) != hipSuccess) return fail(SW_ERR_HIP, std::string("sw_mask_subjects: launch (resolve): ") + hipGetErrorString(e));
        (void)mark(2);
        hipLaunchKernelGGL(swmk::apply_kernel, dim3(unsigned(applyTiles)), dim3(swmk::kThreads), 0, s, chars, out, r, p->window, keep,
                           out == chars ? 1 : 0, counts);
        if ((e = hipGetLastError()) != hipSuccess) return fail(SW_ERR_HIP, std::string("sw_mask_subjects: launch (apply): ") + hipGetErrorString(e));
        if ((e = mark(3)) != hipSuccess) return fail(SW_ERR_HIP, std::string("sw_mask_subjects_phases: hipEventRecord: ") + hipGetErrorString(e));
    }
    return SW_OK;
}

extern "C" int sw_mask_subjects(sw_ctx* ctx, const int8_t* chars, const uint64_t* offsets, const int32_t* lengths, int32_t n,
                                const sw_mask_params* p, int8_t* out, void* temp, size_t temp_bytes, size_t* temp_bytes_needed,
                                unsigned long long* counts, void* stream) {
    return mask_subjects(ctx, chars, offsets, lengths, n, p, out, temp, temp_bytes, temp_bytes_needed, counts, stream, nullptr);
}

extern "C" int sw_mask_subjects_phases(sw_ctx* ctx, const int8_t* chars, const uint64_t* offsets, const int32_t* lengths, int32_t n,
                                       const sw_mask_params* p, int8_t* out, void* temp, size_t temp_bytes, unsigned long long* counts,
                                       void* stream, void* const* phase_events) {
    if (!phase_events || !phase_events[0] || !phase_events[1] || !phase_events[2] || !phase_events[3] || !temp)
        return swi::fail(SW_ERR_INVALID, "sw_mask_subjects_phases: four events and the scratch are required");
    return mask_subjects(ctx, chars, offsets, lengths, n, p, out, temp, temp_bytes, nullptr, counts, stream, phase_events);
}
