// sw_msa_select.hip — sw_msa_select (include/cudasw4_amd_msa_select.h): the host side of the selection kernels
// (sw_msa_select_kernel.hpp).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/cudasw4_amd_msa_select.h"
#include "sw_internal.hpp"
#include "sw_msa_select_kernel.hpp"

namespace {
int hip_fail(hipError_t e, const char* what) {
    return swi::fail(SW_ERR_HIP, std::string("sw_msa_select: ") + what + ": " + hipGetErrorString(e));
}
size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }
}  // namespace

extern "C" int sw_msa_select(sw_ctx* ctx, const sw_msa_select_args* a) {
    using swi::fail;
    if (!ctx || !a) return fail(SW_ERR_INVALID, "sw_msa_select: null argument");
    if (a->qlen < 1 || a->qlen > SW_PSSM_MAX_QUERY_LEN)
        return fail(SW_ERR_INVALID, "sw_msa_select: qlen must lie in [1, SW_PSSM_MAX_QUERY_LEN]");
    if (a->n < 0 || a->n > SW_MSA_SELECT_MAX_HITS) return fail(SW_ERR_INVALID, "sw_msa_select: n must lie in [0, SW_MSA_SELECT_MAX_HITS]");
    if (a->min_coverage < 0 || a->min_coverage > 100) return fail(SW_ERR_INVALID, "sw_msa_select: min_coverage must lie in [0, 100]");
    if (a->min_query_identity < 0 || a->min_query_identity > 100)
        return fail(SW_ERR_INVALID, "sw_msa_select: min_query_identity must lie in [0, 100]");
    if (a->min_query_identity > 0 && !a->query) return fail(SW_ERR_INVALID, "sw_msa_select: min_query_identity needs a query");
    if (a->diff < 0) return fail(SW_ERR_INVALID, "sw_msa_select: diff must not be negative");
    if (a->n_ladder < 1 || a->n_ladder > SW_MSA_SELECT_MAX_LADDER || !a->ladder)
        return fail(SW_ERR_INVALID, "sw_msa_select: the ladder needs 1 .. 16 rungs");
    for (int k = 0; k < a->n_ladder; k++)
        if (a->ladder[k] < 1 || a->ladder[k] > 100 || (k > 0 && a->ladder[k] <= a->ladder[k - 1]))
            return fail(SW_ERR_INVALID, "sw_msa_select: the rungs must lie in [1, 100] and ascend strictly");
    if (!a->state || !a->residues || !a->counts) return fail(SW_ERR_INVALID, "sw_msa_select: null output buffer");
    if (a->n > 0 && (!a->chars || !a->offsets || !a->lengths || !a->results || !a->cigar))
        return fail(SW_ERR_INVALID, "sw_msa_select: null hit buffer");
    // temp, every part behind a multiple of 256 bytes: the planes, pairs, ident(master, .), the thresholds, the levels of all
    // ordered pairs, the select kernel's depth and thin mask
    const size_t rows = (size_t)a->n + 1;
    const size_t rpad = round_up(rows, sws::kTile);
    const size_t words = ((size_t)a->qlen + 31) / 32;
    const size_t wpad = round_up(words, sws::kWords);
    const size_t plane_bytes = round_up(wpad * sws::kPlanes * rpad * sizeof(uint32_t), 256);
    const size_t row_bytes = round_up(rpad * sizeof(int32_t), 256);
    const size_t thr_bytes = round_up((size_t)a->n_ladder * rpad * sizeof(int32_t), 256);
    const size_t level_bytes = round_up(rpad * rpad, 256);
    const size_t depth_bytes = round_up((size_t)a->qlen * sizeof(int32_t), 256);
    const size_t thin_bytes = round_up(round_up(words, 2) * sizeof(uint32_t), 256);
    const size_t need = plane_bytes + 2 * row_bytes + thr_bytes + level_bytes + depth_bytes + thin_bytes;
    if (a->temp_bytes_needed) *a->temp_bytes_needed = need;
    if (!a->temp) return SW_OK;
    if (a->temp_bytes < need) return fail(SW_ERR_TEMP, "sw_msa_select: temp buffer too small (see temp_bytes_needed)");
    if (reinterpret_cast<uintptr_t>(a->temp) % 8 != 0) return fail(SW_ERR_INVALID, "sw_msa_select: temp must be 8-byte aligned");
    hipError_t e = hipSetDevice(swi::device_of(ctx));
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    hipStream_t stream = static_cast<hipStream_t>(a->stream);
    auto record = [&](int i) -> hipError_t {
        return a->phase_events ? hipEventRecord(static_cast<hipEvent_t>(a->phase_events[i]), stream) : hipSuccess;
    };
    if ((e = record(0)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    char* at = static_cast<char*>(a->temp);
    auto take = [&](size_t bytes) {
        char* here = at;
        at += bytes;
        return here;
    };
    sws::SelectParams p{};
    p.hits.query = a->query;
    p.hits.qlen = a->qlen;
    p.hits.n = a->n;
    p.hits.chars = a->chars;
    p.hits.offsets = a->offsets;
    p.hits.lengths = a->lengths;
    p.hits.results = a->results;
    p.hits.cigar = a->cigar;
    p.hits.include = a->include;
    p.min_coverage = a->min_coverage;
    p.min_query_identity = a->min_query_identity;
    p.diff = a->diff;
    p.n_ladder = a->n_ladder;
    for (int k = 0; k < a->n_ladder; k++) p.ladder[k] = a->ladder[k];
    p.rows = a->rows;
    p.residues = a->residues;
    p.state = a->state;
    p.counts = a->counts;
    p.depth_out = a->depth;
    p.levels_out = a->levels;
    p.planes = reinterpret_cast<uint32_t*>(take(plane_bytes));
    p.pairs = reinterpret_cast<int32_t*>(take(row_bytes));
    p.mident = reinterpret_cast<int32_t*>(take(row_bytes));
    p.thr = reinterpret_cast<int32_t*>(take(thr_bytes));
    p.levels = reinterpret_cast<uint8_t*>(take(level_bytes));
    p.depth = reinterpret_cast<int32_t*>(take(depth_bytes));
    p.thin = reinterpret_cast<uint32_t*>(take(thin_bytes));
    p.words = (int32_t)words;
    p.wpad = (int32_t)wpad;
    p.rpad = (int32_t)rpad;
    // the rows kernel writes every plane word and threshold of a real row; what is left is the padding: zero planes, and
    // thresholds nothing reaches
    if ((e = hipMemsetAsync(p.planes, 0, plane_bytes, stream)) != hipSuccess) return hip_fail(e, "hipMemsetAsync");
    if ((e = hipMemsetAsync(p.thr, 0x7f, thr_bytes, stream)) != hipSuccess) return hip_fail(e, "hipMemsetAsync");
    hipLaunchKernelGGL(sws::msa_select_rows_kernel, dim3((unsigned)rows), dim3(sws::kLanes), 0, stream, p);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "launch (rows)");
    if ((e = record(1)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    {
        const unsigned tiles = (unsigned)(rpad / sws::kTile);
        const dim3 grid((tiles + sws::kPairWaves - 1) / sws::kPairWaves, tiles), block(sws::kPairWaves * sws::kLanes);
        if (a->n_ladder <= 2) hipLaunchKernelGGL(sws::msa_levels_kernel<2>, grid, block, 0, stream, p);
        else if (a->n_ladder <= 8) hipLaunchKernelGGL(sws::msa_levels_kernel<8>, grid, block, 0, stream, p);
        else hipLaunchKernelGGL(sws::msa_levels_kernel<16>, grid, block, 0, stream, p);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "launch (levels)");
        if (a->levels) {
            hipLaunchKernelGGL(sws::msa_levels_out_kernel, dim3((unsigned)((rows + 255) / 256), (unsigned)rows), dim3(256), 0, stream, p);
            if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "launch (levels out)");
        }
    }
    if ((e = record(2)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    hipLaunchKernelGGL(sws::msa_select_kernel, dim3(1), dim3(sws::kSelectThreads), 0, stream, p);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "launch (select)");
    if (a->depth) {
        hipLaunchKernelGGL(sws::msa_depth_kernel, dim3((unsigned)words), dim3(sws::kDepthGroups * 32), 0, stream, p);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "launch (depth)");
    }
    if ((e = record(3)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    return SW_OK;
}
