// sw_align.hip — sw_align_hits (include/cudasw4_amd.h) and sw_align_hits_pssm (include/cudasw4_amd_pssm.h): the host side
// of the hit-alignment kernels (sw_align_kernel.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/cudasw4_amd.h"
#include "../../include/cudasw4_amd_pssm.h"
#include "sw_align_kernel.hpp"
#include "sw_internal.hpp"

namespace {

constexpr size_t kAlign = 256;
size_t round_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

int hip_fail(hipError_t e, const char* what) { return swi::fail(SW_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

// both entry points.  pssm == nullptr: the letter form (a->query scored with the context's matrix); else a->query is the
// consensus (may be null) and the rows of `pssm` are the scores.  `name` opens the error messages.
int align_hits(sw_ctx* ctx, const sw_align_args* a, const int8_t* pssm, const std::string& name) {
    using swi::fail;
    const bool letters = pssm == nullptr;
    if (a->qlen <= 0 || a->n < 0) return fail(SW_ERR_INVALID, name + ": qlen must be positive and n not negative");
    if (a->gop > 0 || a->gex > 0 || a->gop < -(1 << 16) || a->gex < -(1 << 16))
        return fail(SW_ERR_INVALID, name + ": gap scores must lie in [-65536, 0]");
    if (a->max_subject_len < 0 || a->max_subject_len > SW_MAX_SUBJECT_LEN)
        return fail(SW_ERR_INVALID, name + ": max_subject_len out of range");
    if (a->qlen > (1 << 20)) return fail(SW_ERR_INVALID, name + ": queries longer than 2^20 residues are not supported");
    int dim = 0;
    const int8_t* matrix = letters ? swi::matrix(ctx, &dim) : pssm;
    if (!matrix) return fail(SW_ERR_NO_MATRIX, "sw_set_matrix has not been called");
    const bool coords_only = (a->flags & SW_ALIGN_COORDS_ONLY) != 0;
    if (a->flags & ~SW_ALIGN_COORDS_ONLY) return fail(SW_ERR_INVALID, name + ": unknown flag");
    const size_t border_bytes = round_up(sizeof(int2) * ((size_t)a->max_subject_len + 1));
    const size_t trace_bytes = coords_only ? 0 : round_up(a->trace_bytes);
    const size_t slot = border_bytes + trace_bytes;
    if (!a->temp) {
        if (a->temp_bytes_needed) *a->temp_bytes_needed = slot * (size_t)a->n;
        return SW_OK;
    }
    if (a->n == 0) return SW_OK;
    if ((letters && !a->query) || !a->chars || !a->offsets || !a->lengths || !a->results)
        return fail(SW_ERR_INVALID, name + ": null buffer");
    if (!coords_only && (!a->cigar || !a->cigar_offsets)) return fail(SW_ERR_INVALID, name + ": null CIGAR buffer");
    const size_t chunk = std::min<size_t>((size_t)a->n, a->temp_bytes / slot);
    if (chunk == 0)
        return fail(SW_ERR_TEMP, name + ": temp holds no pair (" + std::to_string(slot) + " bytes per pair)");
    hipError_t e = hipSetDevice(swi::device_of(ctx));
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    hipStream_t stream = static_cast<hipStream_t>(a->stream);
    swa::AlignParams p{};
    p.query = a->query;
    p.qlen = a->qlen;
    p.chars = a->chars;
    p.offsets = a->offsets;
    p.lengths = a->lengths;
    p.max_len = a->max_subject_len;
    p.matrix = matrix;
    p.mrows = letters ? dim + 1 : 0;
    p.gop = a->gop;
    p.gex = a->gex;
    p.expected = a->expected_scores;
    p.results = a->results;
    p.cigar = a->cigar;
    p.cigar_offsets = a->cigar_offsets;
    p.temp = static_cast<char*>(a->temp);
    p.slot_bytes = slot;
    p.border_bytes = border_bytes;
    p.trace_bytes = trace_bytes;
    // phase-major: every pair's (a), then (b), then (c); the results carry what one phase hands to the next
    void (*const letter_phases[3])(swa::AlignParams) = {swa::align_end_kernel<false>, swa::align_start_kernel<false>,
                                                        swa::align_trace_kernel<false>};
    void (*const pssm_phases[3])(swa::AlignParams) = {swa::align_end_kernel<true>, swa::align_start_kernel<true>,
                                                      swa::align_trace_kernel<true>};
    void (*const* phases)(swa::AlignParams) = letters ? letter_phases : pssm_phases;
    auto record = [&](int i) -> hipError_t {
        return a->phase_events ? hipEventRecord(static_cast<hipEvent_t>(a->phase_events[i]), stream) : hipSuccess;
    };
    for (int ph = 0; ph < 3; ph++) {
        if ((e = record(ph)) != hipSuccess) return hip_fail(e, "hipEventRecord");
        if (ph == 2 && coords_only) break;
        for (size_t first = 0; first < (size_t)a->n; first += chunk) {
            p.first = (int32_t)first;
            const unsigned grid = (unsigned)std::min(chunk, (size_t)a->n - first);
            hipLaunchKernelGGL(phases[ph], dim3(grid), dim3(swa::kLanes), 0, stream, p);
            e = hipGetLastError();
            if (e != hipSuccess) return hip_fail(e, (name + " launch").c_str());
        }
    }
    if ((e = record(3)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    return SW_OK;
}

}  // namespace

extern "C" int sw_align_hits(sw_ctx* ctx, const sw_align_args* a) {
    if (!ctx || !a) return swi::fail(SW_ERR_INVALID, "sw_align_hits: null argument");
    return align_hits(ctx, a, nullptr, "sw_align_hits");
}

extern "C" int sw_align_hits_pssm(sw_ctx* ctx, const sw_align_args* a, const int8_t* pssm) {
    if (!ctx || !a || !pssm) return swi::fail(SW_ERR_INVALID, "sw_align_hits_pssm: null argument");
    return align_hits(ctx, a, pssm, "sw_align_hits_pssm");
}
