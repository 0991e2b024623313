// sw_align_hsps.hip — sw_align_hsps / sw_align_hsps_pssm (include/cudasw4_amd_hsps.h): up to max_hsps non-overlapping local
// alignments per pair, in rounds of the three hit-alignment phases (sw_align_kernel.hpp: the hsp_* kernels).
//
// A translation unit of its own: sw_align.hip keeps instantiating exactly the six kernels it did, each dp_pass with its one
// caller, so the code of sw_align_hits does not depend on anything here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/cudasw4_amd.h"
#include "../../include/cudasw4_amd_hsps.h"
#include "sw_align_kernel.hpp"
#include "sw_internal.hpp"

namespace {

constexpr size_t kAlign = 256;
size_t round_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

int hip_fail(hipError_t e, const char* what) { return swi::fail(SW_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

// max_hsps > 1.  pssm == nullptr: the letter form; the argument rules are those of sw_align_hits (sw_align.hip)
int align_rounds(sw_ctx* ctx, const sw_align_args* a, const sw_hsp_args* h, const int8_t* pssm, const std::string& name) {
    using swi::fail;
    const bool letters = pssm == nullptr;
    if (a->qlen <= 0 || a->n < 0) return fail(SW_ERR_INVALID, name + ": qlen must be positive and n not negative");
    if (a->gop > 0 || a->gex > 0 || a->gop < -(1 << 16) || a->gex < -(1 << 16))
        return fail(SW_ERR_INVALID, name + ": gap scores must lie in [-65536, 0]");
    if (a->max_subject_len < 0 || a->max_subject_len > SW_MAX_SUBJECT_LEN)
        return fail(SW_ERR_INVALID, name + ": max_subject_len out of range");
    if (a->qlen > (1 << 20)) return fail(SW_ERR_INVALID, name + ": queries longer than 2^20 residues are not supported");
    if ((int64_t)a->n * h->max_hsps > INT32_MAX) return fail(SW_ERR_INVALID, name + ": n * max_hsps exceeds 2^31 - 1 records");
    int dim = 0;
    const int8_t* matrix = letters ? swi::matrix(ctx, &dim) : pssm;
    if (!matrix) return fail(SW_ERR_NO_MATRIX, "sw_set_matrix has not been called");
    if (a->flags & ~SW_ALIGN_COORDS_ONLY) return fail(SW_ERR_INVALID, name + ": unknown flag");
    const size_t border_bytes = round_up(sizeof(int2) * ((size_t)a->max_subject_len + 1));
    const size_t trace_bytes = round_up(a->trace_bytes);
    // the used pairs of alignments 0 .. max_hsps - 2: one int32 per query row each, behind the direction bits
    const size_t used_bytes = round_up(sizeof(int32_t) * (size_t)(h->max_hsps - 1) * (size_t)a->qlen);
    const size_t slot = border_bytes + trace_bytes + used_bytes;
    if (!a->temp) {
        if (a->temp_bytes_needed) *a->temp_bytes_needed = slot * (size_t)a->n;
        return SW_OK;
    }
    if (a->n == 0) return SW_OK;
    if ((letters && !a->query) || !a->chars || !a->offsets || !a->lengths || !a->results)
        return fail(SW_ERR_INVALID, name + ": null buffer");
    if (!a->cigar || !a->cigar_offsets) return fail(SW_ERR_INVALID, name + ": null CIGAR buffer");
    const size_t chunk = std::min<size_t>((size_t)a->n, a->temp_bytes / slot);
    if (chunk == 0)
        return fail(SW_ERR_TEMP, name + ": temp holds no pair (" + std::to_string(slot) + " bytes per pair)");
    hipError_t e = hipSetDevice(swi::device_of(ctx));
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    hipStream_t stream = static_cast<hipStream_t>(a->stream);
    swa::HspParams hp{};
    swa::AlignParams& p = hp.a;
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
    hp.max_hsps = h->max_hsps;
    hp.min_score = h->min_score;
    hp.used_off = border_bytes + trace_bytes;
    // [score source][round 0 / vetoed rounds][phase]
    using Kernel = void (*)(swa::HspParams);
    static const Kernel kernels[2][2][3] = {
        {{swa::hsp_end_kernel<false, false>, swa::hsp_start_kernel<false, false>, swa::hsp_trace_kernel<false, false>},
         {swa::hsp_end_kernel<false, true>, swa::hsp_start_kernel<false, true>, swa::hsp_trace_kernel<false, true>}},
        {{swa::hsp_end_kernel<true, false>, swa::hsp_start_kernel<true, false>, swa::hsp_trace_kernel<true, false>},
         {swa::hsp_end_kernel<true, true>, swa::hsp_start_kernel<true, true>, swa::hsp_trace_kernel<true, true>}}};
    // chunk by chunk (the used pairs live in the chunk's scratch); within a chunk round-major and phase-major: every
    // pair's (a), then (b), then (c), then the next round.  The records carry what one launch hands to the next.
    for (size_t first = 0; first < (size_t)a->n; first += chunk) {
        p.first = (int32_t)first;
        const unsigned grid = (unsigned)std::min(chunk, (size_t)a->n - first);
        for (int32_t round = 0; round < h->max_hsps; round++) {
            hp.round = round;
            for (int ph = 0; ph < 3; ph++) {
                hipLaunchKernelGGL(kernels[letters ? 0 : 1][round ? 1 : 0][ph], dim3(grid), dim3(swa::kLanes), 0, stream, hp);
                e = hipGetLastError();
                if (e != hipSuccess) return hip_fail(e, (name + " launch").c_str());
            }
        }
    }
    return SW_OK;
}

// the rules of sw_hsp_args first (they need no device); max_hsps == 1 is the plain call
int align_hsps(sw_ctx* ctx, const sw_align_args* a, const sw_hsp_args* h, const int8_t* pssm, bool want_pssm,
               const std::string& name) {
    using swi::fail;
    if (!a || !h) return fail(SW_ERR_INVALID, name + ": null argument");
    if (h->max_hsps < 1 || h->max_hsps > SW_MAX_HSPS)
        return fail(SW_ERR_INVALID, name + ": max_hsps must lie in [1, " + std::to_string(SW_MAX_HSPS) + "]");
    if (h->min_score < 1) return fail(SW_ERR_INVALID, name + ": min_score must be at least 1");
    if (h->max_hsps > 1 && (a->flags & SW_ALIGN_COORDS_ONLY))
        return fail(SW_ERR_INVALID, name + ": SW_ALIGN_COORDS_ONLY needs max_hsps == 1 (without a traceback there are no pairs to exclude)");
    if (h->max_hsps > 1 && a->phase_events) return fail(SW_ERR_INVALID, name + ": phase_events needs max_hsps == 1");
    if (!ctx || (want_pssm && !pssm)) return fail(SW_ERR_INVALID, name + ": null argument");
    if (h->max_hsps == 1) return want_pssm ? sw_align_hits_pssm(ctx, a, pssm) : sw_align_hits(ctx, a);
    return align_rounds(ctx, a, h, pssm, name);
}

}  // namespace

extern "C" int sw_align_hsps(sw_ctx* ctx, const sw_align_args* a, const sw_hsp_args* h) {
    return align_hsps(ctx, a, h, nullptr, false, "sw_align_hsps");
}

extern "C" int sw_align_hsps_pssm(sw_ctx* ctx, const sw_align_args* a, const sw_hsp_args* h, const int8_t* pssm) {
    return align_hsps(ctx, a, h, pssm, true, "sw_align_hsps_pssm");
}
