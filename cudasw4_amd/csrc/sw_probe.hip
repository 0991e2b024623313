// sw_probe.hip — probes and micro-runs of the C ABI: the start handshake in miniature (sw_probe_handshake), whether two
// streams run side by side (sw_streams_run_concurrently) and the VALU issue-rate micro-benchmark (sw_measure_valu_rate).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <ctime>
#include <string>
#include <vector>

#include "../../include/cudasw4_amd.h"
#include "sw_ctx.hpp"

using swi::fail;

namespace {
// Issue-rate micro-runs (tools/ubench/valu_rate.hip, mix_rate.hip in-process): `iters` iterations of 32 independent
// instructions of the kind's inner-loop mix on every lane of 16 waves per CU; every wave also reports how many shader-clock
// ticks (s_memtime) went by per 100 MHz tick (s_memrealtime): the clock the chip actually held during the run.
#define SW_REP8(OP) OP(0) OP(1) OP(2) OP(3) OP(4) OP(5) OP(6) OP(7)
#define SW_OP_PK_MAX3(i) asm volatile("v_pk_maximum3_f16 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
#define SW_OP_ADD_F32(i) asm volatile("v_add_f32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
#define SW_OP_MAX3_F32(i) asm volatile("v_max3_f32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
#define SW_OP_ADD_U32(i) asm volatile("v_add_u32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
#define SW_OP_MAX3_I32(i) asm volatile("v_max3_i32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
#define SW_OP_PK_FMA(i) asm volatile("v_pk_fma_f16 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,0,1]" : "+v"(a[i]) : "v"(b), "v"(c));
#define SW_OP_PK_ADD(i) asm volatile("v_pk_add_f16 %0, %0, %1" : "+v"(a[i]) : "v"(b));
#define SW_OP_DPP(i) asm volatile("v_mov_b32_dpp %0, %1 row_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(a[i]) : "v"(b));
#define SW_OP_PERM(i) asm volatile("v_perm_b32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
template <int MIX>
__global__ void __launch_bounds__(256) valu_rate_kernel(unsigned* out, unsigned long long* clocks, unsigned seed, int iters) {
    unsigned a[8];
    unsigned b = seed + threadIdx.x, c = seed * 3u + 1u;
    for (int i = 0; i < 8; i++) a[i] = seed + i + threadIdx.x;
    if constexpr (MIX == 4) {
        asm volatile("v_mov_b32 v0, %0\nv_mov_b32 v1, %0\nv_mov_b32 v2, %0\nv_mov_b32 v3, %0\nv_mov_b32 v4, %0\nv_mov_b32 v5, %0\nv_mov_b32 v6, %0\nv_mov_b32 v7, %0\n"
                     "v_mov_b32 v8, %1\nv_mov_b32 v9, %1\nv_mov_b32 v10, %1\nv_mov_b32 v11, %1\nv_mov_b32 v12, %2\nv_mov_b32 v13, %2\nv_mov_b32 v14, %2\nv_mov_b32 v15, %2\n"
                     :: "v"(a[0]), "v"(b), "v"(c) : "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15");
    }
    const unsigned long long t0 = clock64(), w0 = wall_clock64();
    for (int it = 0; it < iters; it++) {
        if constexpr (MIX == 0) { SW_REP8(SW_OP_PK_MAX3) SW_REP8(SW_OP_PK_MAX3) SW_REP8(SW_OP_PK_MAX3) SW_REP8(SW_OP_PK_MAX3) }
        // fp32 kind: 4 v_add_f32 : 3.5 v_max3_f32 per cell = 16 : 14 + 2 to fill the 32
        if constexpr (MIX == 1) { SW_REP8(SW_OP_ADD_F32) SW_REP8(SW_OP_MAX3_F32) SW_REP8(SW_OP_ADD_F32) SW_OP_MAX3_F32(0) SW_OP_MAX3_F32(1) SW_OP_MAX3_F32(2) SW_OP_MAX3_F32(3) SW_OP_MAX3_F32(4) SW_OP_MAX3_F32(5) SW_OP_ADD_F32(6) SW_OP_ADD_F32(7) }
        // int32 kind: 2.25 v_add_u32 : 3.5 v_max3_i32 per cell ~ 12 : 20
        // the packed kernels' OWN mix (static histogram of the dominant loop body, sw_scan_kernel<f16x2, R = 32, 16 lanes, multi-stripe>,
        // per four steps: 128 v_pk_fma_f16, 454 v_pk_maximum3_f16, 164 v_pk_add_f16 and ~76 others — DPP moves, v_perm_b32, address
        // adds — of 822): in 64 slots 10 fma, 35 max3, 13 add, 3 DPP, 2 v_add_u32, 1 v_perm.  A pure v_pk_maximum3_f16 stream issues
        // FEWER lane-instructions per second than the kernel does (round 5: frac_of_measured_peak 1.06), this one cannot be beaten
        // by a loop of the same composition that also waits for LDS and neighbours
        if constexpr (MIX == 3) {
            SW_REP8(SW_OP_PK_MAX3) SW_OP_PK_FMA(0) SW_OP_PK_FMA(1) SW_OP_PK_ADD(2) SW_OP_PK_ADD(3) SW_OP_DPP(4) SW_OP_PK_FMA(5) SW_OP_PK_ADD(6) SW_OP_ADD_U32(7)
            SW_REP8(SW_OP_PK_MAX3) SW_OP_PK_FMA(0) SW_OP_PK_FMA(1) SW_OP_PK_ADD(2) SW_OP_PK_ADD(3) SW_OP_DPP(4) SW_OP_PK_FMA(5) SW_OP_PK_ADD(6) SW_OP_PERM(7)
            SW_REP8(SW_OP_PK_MAX3) SW_OP_PK_FMA(0) SW_OP_PK_FMA(1) SW_OP_PK_ADD(2) SW_OP_PK_ADD(3) SW_OP_DPP(4) SW_OP_PK_ADD(5) SW_OP_PK_ADD(6) SW_OP_ADD_U32(7)
            SW_REP8(SW_OP_PK_MAX3) SW_OP_PK_FMA(0) SW_OP_PK_FMA(1) SW_OP_PK_ADD(2) SW_OP_PK_ADD(3) SW_OP_PK_MAX3(4) SW_OP_PK_MAX3(5) SW_OP_PK_MAX3(6) SW_OP_PK_ADD(7)
        }
        // mix 4: mix 3's composition with every instruction's three sources in three different register banks (bank = register
        // number mod 4) — explicit registers: accumulators v0..v7, the second operand from v8..v11, the third from v12..v15.
        // With operands wherever the allocator puts them a VOP3(P) instruction whose sources meet in one bank takes an extra
        // cycle: mixes 0 and 3 sustain 58-59.5 lanes/clk/CU, less than the scan kernels themselves, whose registers hipcc assigns
        // with the banks in mind.
        if constexpr (MIX == 4) {
#define SW_B4_MAX3(i, j, k) "v_pk_maximum3_f16 v" #i ", v" #i ", v" #j ", v" #k "\n"
#define SW_B4_FMA(i, j, k) "v_pk_fma_f16 v" #i ", v" #j ", v" #k ", v" #i " op_sel:[0,1,0] op_sel_hi:[1,0,1]\n"
#define SW_B4_ADD(i, j) "v_pk_add_f16 v" #i ", v" #i ", v" #j "\n"
#define SW_B4_DPP(i, j) "v_mov_b32_dpp v" #i ", v" #j " row_shr:1 row_mask:0xf bank_mask:0xf\n"
#define SW_B4_ADDU(i, j) "v_add_u32 v" #i ", v" #i ", v" #j "\n"
#define SW_B4_ROW8 SW_B4_MAX3(0, 9, 14) SW_B4_MAX3(1, 10, 15) SW_B4_MAX3(2, 11, 12) SW_B4_MAX3(3, 8, 13) SW_B4_MAX3(4, 9, 14) SW_B4_MAX3(5, 10, 15) SW_B4_MAX3(6, 11, 12) SW_B4_MAX3(7, 8, 13)
            asm volatile(
                SW_B4_ROW8 SW_B4_FMA(0, 9, 14) SW_B4_FMA(1, 10, 15) SW_B4_ADD(2, 11) SW_B4_ADD(3, 8) SW_B4_DPP(4, 9) SW_B4_FMA(5, 10, 15) SW_B4_ADD(6, 11) SW_B4_ADDU(7, 8)
                SW_B4_ROW8 SW_B4_FMA(0, 9, 14) SW_B4_FMA(1, 10, 15) SW_B4_ADD(2, 11) SW_B4_ADD(3, 8) SW_B4_DPP(4, 9) SW_B4_FMA(5, 10, 15) SW_B4_ADD(6, 11) SW_B4_MAX3(7, 8, 13)
                SW_B4_ROW8 SW_B4_FMA(0, 9, 14) SW_B4_FMA(1, 10, 15) SW_B4_ADD(2, 11) SW_B4_ADD(3, 8) SW_B4_DPP(4, 9) SW_B4_ADD(5, 10) SW_B4_ADD(6, 11) SW_B4_ADDU(7, 8)
                SW_B4_ROW8 SW_B4_FMA(0, 9, 14) SW_B4_FMA(1, 10, 15) SW_B4_ADD(2, 11) SW_B4_ADD(3, 8) SW_B4_MAX3(4, 9, 14) SW_B4_MAX3(5, 10, 15) SW_B4_MAX3(6, 11, 12) SW_B4_ADD(7, 8)
                ::: "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15");
        }
        if constexpr (MIX == 2) { SW_REP8(SW_OP_MAX3_I32) SW_REP8(SW_OP_ADD_U32) SW_REP8(SW_OP_MAX3_I32) SW_OP_ADD_U32(0) SW_OP_ADD_U32(1) SW_OP_ADD_U32(2) SW_OP_ADD_U32(3) SW_OP_MAX3_I32(4) SW_OP_MAX3_I32(5) SW_OP_MAX3_I32(6) SW_OP_MAX3_I32(7) }
    }
    const unsigned long long t1 = clock64(), w1 = wall_clock64();
    if constexpr (MIX == 4) asm volatile("v_mov_b32 %0, v0\nv_xor_b32 %0, %0, v7" : "=v"(a[0]) :: "v0", "v7");
    unsigned r = 0;
    for (int i = 0; i < 8; i++) r ^= a[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = r;
    if (threadIdx.x == 0) { clocks[2 * blockIdx.x] = t1 - t0; clocks[2 * blockIdx.x + 1] = w1 - w0; }
}
}  // namespace

extern "C" {

namespace {
__global__ void probe_wait_kernel(unsigned* flag, unsigned* saw, unsigned long long max_ticks) {
    const unsigned long long t0 = wall_clock64();
    unsigned v = 0;
    while ((v = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0 && wall_clock64() - t0 < max_ticks)
        __builtin_amdgcn_s_sleep(8);
    *saw = v;
}
__global__ void probe_set_kernel(unsigned* flag) { __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the side launch of the start handshake in miniature: count in (what releases the gated stream), then stay resident — for a
// bounded time — until the gated kernel has been seen to run
__global__ void probe_side_kernel(unsigned* signal, unsigned* flag, unsigned* saw, unsigned long long max_ticks) {
    __hip_atomic_fetch_add(signal, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    const unsigned long long t0 = wall_clock64();
    unsigned v = 0;
    while ((v = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0 && wall_clock64() - t0 < max_ticks)
        __builtin_amdgcn_s_sleep(8);
    *saw = v;
}
}  // namespace

int sw_probe_handshake(sw_ctx* ctx, void* side_stream, void* gated_stream, uint32_t* signal) {
    if (!ctx || !signal) return fail(SW_ERR_INVALID, "null argument");
    SW_HIP(hipSetDevice(ctx->device));
    hipStream_t side = static_cast<hipStream_t>(side_stream), gated = static_cast<hipStream_t>(gated_stream);
    unsigned* words = reinterpret_cast<unsigned*>(ctx->d_zeros + 72);  // (flag, saw): two spare words of the context's constant block
    SW_HIP(hipStreamSynchronize(side));
    SW_HIP(hipStreamSynchronize(gated));
    SW_HIP(hipMemsetAsync(words, 0, 2 * sizeof(unsigned), side));
    SW_HIP(hipStreamSynchronize(side));
    const uint32_t base = *reinterpret_cast<volatile uint32_t*>(signal);   // signal memory is host-visible
    SW_HIP(hipStreamWaitValue32(gated, signal, base + 1u, hipStreamWaitValueGte, 0xffffffffu));
    hipLaunchKernelGGL(probe_set_kernel, dim3(1), dim3(1), 0, gated, words);
    hipLaunchKernelGGL(probe_side_kernel, dim3(1), dim3(1), 0, side, signal, words, words + 1, 1000000ull);  // 100 MHz ticks: 10 ms
    SW_HIP(hipGetLastError());
    // the gated stream must get through within a bounded time; if its wait is never released (a profiler that serialises
    // kernels, a runtime without working wait-value packets) the host releases it by hand
    bool released = true;
    for (int i = 0;; i++) {
        const hipError_t q = hipStreamQuery(gated);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) return fail(SW_ERR_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(q));
        if (i >= 2000) {   // ~2 s
            *reinterpret_cast<volatile uint32_t*>(signal) = base + 1u;
            released = false;
            break;
        }
        struct timespec ts = {0, 1000000};
        nanosleep(&ts, nullptr);
    }
    SW_HIP(hipStreamSynchronize(side));
    SW_HIP(hipStreamSynchronize(gated));
    unsigned saw = 0;
    SW_HIP(hipMemcpy(&saw, words + 1, sizeof(unsigned), hipMemcpyDeviceToHost));
    *reinterpret_cast<volatile uint32_t*>(signal) = base;
    return released && saw ? 1 : 0;
}

int sw_streams_run_concurrently(sw_ctx* ctx, void* stream_a, void* stream_b) {
    if (!ctx) return fail(SW_ERR_INVALID, "null context");
    SW_HIP(hipSetDevice(ctx->device));
    // a kernel on stream A waits (at most ~5 ms) for a word that a kernel on stream B sets: it sees the word only if the
    // second kernel could start while the first one was still running, i.e. if the runtime did not put both streams on
    // one hardware queue
    unsigned* words = reinterpret_cast<unsigned*>(ctx->d_zeros + 72);  // two spare words of the context's constant block
    SW_HIP(hipMemsetAsync(words, 0, 2 * sizeof(unsigned), static_cast<hipStream_t>(stream_a)));
    SW_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream_a)));
    hipLaunchKernelGGL(probe_wait_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream_a), words, words + 1, 500000ull);  // 100 MHz ticks
    hipLaunchKernelGGL(probe_set_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream_b), words);
    SW_HIP(hipGetLastError());
    unsigned saw = 0;
    SW_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream_b)));
    SW_HIP(hipMemcpyAsync(&saw, words + 1, sizeof(unsigned), hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream_a)));
    SW_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream_a)));
    return saw ? 1 : 0;
}

int sw_measure_valu_rate(sw_ctx* ctx, int mix, int millis, double* lane_instr_per_s, double* shader_hz) {
    if (!ctx || mix < 0 || mix > 4) return fail(SW_ERR_INVALID, "null context or unknown instruction mix");
    SW_HIP(hipSetDevice(ctx->device));
    const int grid = std::max(1, ctx->plan.num_cus) * 4;   // 16 waves per CU: four per SIMD
    unsigned* out = nullptr;
    unsigned long long* clocks = nullptr;
    SW_HIP(hipMalloc(&out, (size_t)grid * 256 * sizeof(unsigned)));
    if (hipMalloc(&clocks, (size_t)grid * 2 * sizeof(unsigned long long)) != hipSuccess) { (void)hipFree(out); return fail(SW_ERR_HIP, "hipMalloc"); }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t err = hipEventCreate(&e0);
    if (err == hipSuccess) err = hipEventCreate(&e1);
    auto run = [&](int iters, float* ms) -> hipError_t {
        hipError_t e = hipEventRecord(e0, nullptr);
        if (e != hipSuccess) return e;
        if (mix == 0) hipLaunchKernelGGL(valu_rate_kernel<0>, dim3(grid), dim3(256), 0, nullptr, out, clocks, 7u, iters);
        else if (mix == 1) hipLaunchKernelGGL(valu_rate_kernel<1>, dim3(grid), dim3(256), 0, nullptr, out, clocks, 7u, iters);
        else if (mix == 2) hipLaunchKernelGGL(valu_rate_kernel<2>, dim3(grid), dim3(256), 0, nullptr, out, clocks, 7u, iters);
        else if (mix == 3) hipLaunchKernelGGL(valu_rate_kernel<3>, dim3(grid), dim3(256), 0, nullptr, out, clocks, 7u, iters);
        else hipLaunchKernelGGL(valu_rate_kernel<4>, dim3(grid), dim3(256), 0, nullptr, out, clocks, 7u, iters);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(ms, e0, e1);
        return e;
    };
    float ms = 0.0f;
    int iters = 4096;
    if (err == hipSuccess) err = run(iters, &ms);          // warm-up and calibration
    if (err == hipSuccess && ms > 0.0f) {
        iters = (int)std::min(1.0e7, std::max(1024.0, iters * (double)std::max(millis, 1) / ms));
        err = run(iters, &ms);
    }
    double hz = 0.0;
    if (err == hipSuccess) {
        std::vector<unsigned long long> h((size_t)grid * 2);
        err = hipMemcpy(h.data(), clocks, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        double ticks = 0.0, wall = 0.0;
        for (int i = 0; i < grid; i++) { ticks += (double)h[2 * i]; wall += (double)h[2 * i + 1]; }
        if (wall > 0.0) hz = ticks / wall * 100.0e6;   // s_memrealtime counts at 100 MHz
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(out);
    (void)hipFree(clocks);
    if (err != hipSuccess) return fail(SW_ERR_HIP, std::string("sw_measure_valu_rate: ") + hipGetErrorString(err));
    if (lane_instr_per_s) *lane_instr_per_s = ms > 0.0f ? (double)grid * 256.0 * (mix >= 3 ? 64.0 : 32.0) * (double)iters / (ms * 1e-3) : 0.0;
    if (shader_hz) *shader_hz = hz;
    return SW_OK;
}

}  // extern "C"
