// sw_shuffle.hip — sw_shuffle_subjects (include/cudasw4_amd_shuffle.h): the host side of the shuffle kernel
// (sw_shuffle_kernel.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/cudasw4_amd_shuffle.h"
#include "sw_internal.hpp"
#include "sw_shuffle_kernel.hpp"

extern "C" int sw_shuffle_subjects(sw_ctx* ctx, const int8_t* chars, const uint64_t* offsets, const int32_t* lengths,
                                   const int64_t* keys, int32_t n, uint32_t seed, int32_t first_replica, int32_t replicas,
                                   int8_t* out, size_t replica_stride, void* stream) {
    using swi::fail;
    if (!ctx) return fail(SW_ERR_INVALID, "sw_shuffle_subjects: null context");
    if (n < 0 || replicas < 0 || first_replica < 0) return fail(SW_ERR_INVALID, "sw_shuffle_subjects: n, replicas and first_replica must not be negative");
    if (replica_stride % 4 != 0) return fail(SW_ERR_INVALID, "sw_shuffle_subjects: replica_stride must be a multiple of 4");
    if (n == 0 || replicas == 0) return SW_OK;
    if (!chars || !offsets || !lengths || !out) return fail(SW_ERR_INVALID, "sw_shuffle_subjects: null pointer");
    if (reinterpret_cast<uintptr_t>(out) % 4 != 0 || reinterpret_cast<uintptr_t>(offsets) % 8 != 0 ||
        reinterpret_cast<uintptr_t>(lengths) % 4 != 0 || reinterpret_cast<uintptr_t>(keys) % 8 != 0)
        return fail(SW_ERR_INVALID, "sw_shuffle_subjects: out and lengths must be 4-byte aligned, offsets and keys 8-byte aligned");
    hipError_t e = hipSetDevice(swi::device_of(ctx));
    if (e != hipSuccess) return fail(SW_ERR_HIP, std::string("sw_shuffle_subjects: hipSetDevice: ") + hipGetErrorString(e));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the two ends of the block: its size decides the grid and whether the stride holds a replica
    uint64_t ends[2] = {0, 0};
    if ((e = hipMemcpyAsync(&ends[0], offsets, sizeof(uint64_t), hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipMemcpyAsync(&ends[1], offsets + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
        return fail(SW_ERR_HIP, std::string("sw_shuffle_subjects: reading the block's ends: ") + hipGetErrorString(e));
    if (ends[1] < ends[0] || (ends[1] - ends[0]) % 4 != 0)
        return fail(SW_ERR_INVALID, "sw_shuffle_subjects: offsets must ascend and the block must be a multiple of 4 bytes");
    const uint64_t blockBytes = ends[1] - ends[0];
    if (uint64_t(replica_stride) < blockBytes) return fail(SW_ERR_INVALID, "sw_shuffle_subjects: replica_stride is smaller than the block");
    if (blockBytes == 0) return SW_OK;
    const uint64_t tiles = (blockBytes + swsh::kTileBytes - 1) / swsh::kTileBytes;
    if (tiles > 0x7fffffffull) return fail(SW_ERR_INVALID, "sw_shuffle_subjects: the block is too large for one call");
    constexpr int32_t kReplicasPerLaunch = 32768;   // (gridDim.y is 16 bits wide)
    for (int32_t r = 0; r < replicas; r += kReplicasPerLaunch) {
        const int32_t count = std::min(kReplicasPerLaunch, replicas - r);
        hipLaunchKernelGGL(swsh::shuffle_subjects_kernel, dim3(unsigned(tiles), unsigned(count)), dim3(swsh::kThreads), 0, s, chars, offsets,
                           lengths, keys, n, blockBytes, seed, uint32_t(first_replica) + uint32_t(r), out + size_t(r) * replica_stride,
                           uint64_t(replica_stride));
        if ((e = hipGetLastError()) != hipSuccess) return fail(SW_ERR_HIP, std::string("sw_shuffle_subjects: launch: ") + hipGetErrorString(e));
    }
    return SW_OK;
}
