// sw_msa.hip — sw_msa_filter (include/cudasw4_amd_msa.h): the host side of the MSA kernels (sw_msa_kernel.hpp).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/cudasw4_amd_msa.h"
#include "sw_internal.hpp"
#include "sw_msa_kernel.hpp"

namespace {
int hip_fail(hipError_t e, const char* what) {
    return swi::fail(SW_ERR_HIP, std::string("sw_msa_filter: ") + what + ": " + hipGetErrorString(e));
}
size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }
}  // namespace

extern "C" int sw_msa_filter(sw_ctx* ctx, const sw_msa_args* a) {
    using swi::fail;
    if (!ctx || !a) return fail(SW_ERR_INVALID, "sw_msa_filter: null argument");
    if (a->qlen < 1 || a->qlen > SW_PSSM_MAX_QUERY_LEN)
        return fail(SW_ERR_INVALID, "sw_msa_filter: qlen must lie in [1, SW_PSSM_MAX_QUERY_LEN]");
    if (a->n < 0 || a->n > SW_MSA_MAX_HITS) return fail(SW_ERR_INVALID, "sw_msa_filter: n must lie in [0, SW_MSA_MAX_HITS]");
    if (a->max_identity < 0 || a->max_identity > 100) return fail(SW_ERR_INVALID, "sw_msa_filter: max_identity must lie in [0, 100]");
    if (!a->residues || !a->keep || !a->purged) return fail(SW_ERR_INVALID, "sw_msa_filter: null output buffer");
    if (a->n > 0 && (!a->chars || !a->offsets || !a->lengths || !a->results || !a->cigar))
        return fail(SW_ERR_INVALID, "sw_msa_filter: null hit buffer");
    // temp: the planes, then the `similar` words (8-byte aligned behind a multiple of 256 bytes)
    const size_t rows = (size_t)a->n + 1;
    const size_t rpad = round_up(rows, swm::kTile);
    const size_t words = ((size_t)a->qlen + 31) / 32;
    const size_t wpad = round_up(words, swm::kWords);
    const size_t plane_bytes = round_up(wpad * swm::kPlanes * rpad * sizeof(uint32_t), 256);
    const bool filter = a->max_identity > 0;
    const size_t similar_bytes = filter ? rpad / swm::kTile * rpad * sizeof(unsigned long long) : 0;
    const size_t need = plane_bytes + similar_bytes;
    if (a->temp_bytes_needed) *a->temp_bytes_needed = need;
    if (!a->temp) return SW_OK;
    if (a->temp_bytes < need) return fail(SW_ERR_TEMP, "sw_msa_filter: temp buffer too small (see temp_bytes_needed)");
    if (reinterpret_cast<uintptr_t>(a->temp) % 8 != 0) return fail(SW_ERR_INVALID, "sw_msa_filter: temp must be 8-byte aligned");
    hipError_t e = hipSetDevice(swi::device_of(ctx));
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    hipStream_t stream = static_cast<hipStream_t>(a->stream);
    auto record = [&](int i) -> hipError_t {
        return a->phase_events ? hipEventRecord(static_cast<hipEvent_t>(a->phase_events[i]), stream) : hipSuccess;
    };
    if ((e = record(0)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    // the rows kernel writes every byte of rows, residues and every plane word of a real row; the greedy kernel every keep
    // byte and purged.  What is left to zero: the padding of the planes and the cells of pair_ident nobody writes.
    if ((e = hipMemsetAsync(a->temp, 0, plane_bytes, stream)) != hipSuccess) return hip_fail(e, "hipMemsetAsync");
    if (a->pair_ident && (e = hipMemsetAsync(a->pair_ident, 0, rows * rows * sizeof(uint32_t), stream)) != hipSuccess)
        return hip_fail(e, "hipMemsetAsync");
    swm::MsaParams p{};
    p.hits.query = a->query;
    p.hits.qlen = a->qlen;
    p.hits.n = a->n;
    p.hits.chars = a->chars;
    p.hits.offsets = a->offsets;
    p.hits.lengths = a->lengths;
    p.hits.results = a->results;
    p.hits.cigar = a->cigar;
    p.hits.include = a->include;
    p.max_identity = a->max_identity;
    p.rows = a->rows;
    p.residues = a->residues;
    p.keep = a->keep;
    p.purged = a->purged;
    p.pair_ident = a->pair_ident;
    p.planes = static_cast<uint32_t*>(a->temp);
    p.similar = filter ? reinterpret_cast<unsigned long long*>(static_cast<char*>(a->temp) + plane_bytes) : nullptr;
    p.words = (int32_t)words;
    p.wpad = (int32_t)wpad;
    p.rpad = (int32_t)rpad;
    hipLaunchKernelGGL(swm::msa_rows_kernel, dim3((unsigned)rows), dim3(swm::kLanes), 0, stream, p);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "launch (rows)");
    if ((e = record(1)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    if (filter || a->pair_ident) {
        const unsigned tiles = (unsigned)(rpad / swm::kTile);
        const dim3 grid((tiles + swm::kPairWaves - 1) / swm::kPairWaves, tiles);
        if (a->pair_ident)
            hipLaunchKernelGGL(swm::msa_pairs_kernel<true>, grid, dim3(swm::kPairWaves * swm::kLanes), 0, stream, p);
        else
            hipLaunchKernelGGL(swm::msa_pairs_kernel<false>, grid, dim3(swm::kPairWaves * swm::kLanes), 0, stream, p);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "launch (pairs)");
    }
    if ((e = record(2)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    hipLaunchKernelGGL(swm::msa_greedy_kernel, dim3(1), dim3(swm::kGreedyWaves * swm::kLanes), 0, stream, p);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "launch (greedy)");
    if ((e = record(3)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    return SW_OK;
}
