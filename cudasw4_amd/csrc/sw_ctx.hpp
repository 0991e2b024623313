// sw_ctx.hpp — the context behind the C ABI's sw_ctx handle, for the translation units that need more of it than the
// swi:: accessors of sw_internal.hpp give (sw_api.hip, sw_topk.hip, sw_probe.hip).  Private: not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/cudasw4_amd.h"
#include "sw_internal.hpp"
#include "sw_plan.hpp"

#define SW_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t e__ = (expr);                                                                  \
        if (e__ != hipSuccess)                                                                    \
            return swi::fail(SW_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));     \
    } while (0)

namespace swi {
// a query profile on the device: the tiles of one (kind, group shape, frame)
struct Profile {
    unsigned char* dev = nullptr;
    size_t capacity = 0;
    bool valid = false;
    int rows = 0, nstripes = 0;  // the query plan it was built for
    int shift = 0;               // added to every substitution score (a = -gex for the column-offset kernels, else 0)
    hipEvent_t ready = nullptr;  // recorded after the build; scans on other streams wait on it
};
constexpr uint32_t kWorkSlots = 4096;
}  // namespace swi

struct sw_ctx {
    int device = 0;
    swp::PlanSettings plan;      // what shapes a launch: device facts, the installed query's length, the tuning of sw_ctx_create
    int8_t* d_matrix = nullptr;  // (dim + 1) x 21: one row per query letter + the padding row, 21 subject letters
    int dim = 21;               // what sw_set_matrix was given: query codes are 0..dim-1
    uint32_t* d_zeros = nullptr; // per kind 64 bytes of its zero pattern (first-stripe border): [kind * 16 words]
    uint32_t* d_work = nullptr;  // kWorkSlots pairs (batch counter of the dynamic batch distribution, started workgroups), one per launch in flight
    uint32_t work_next = 0;
    uint32_t work_zeroed = 0;    // slots from work_next on that sw_set_query has zeroed already (one memset per query instead of one per launch)
    uint32_t* start_signal = nullptr;  // sw_set_start_signal: one-shot, consumed by the next scan / re-score launch
    uint32_t* dry_signal = nullptr;    // sw_set_dry_signal: one-shot as well
    int32_t* dirty_counter = nullptr;  // sw_set_dirty_counter (sticky)
    uint32_t dry_value = 0;
    int grid_reserve = 0;              // sw_set_grid_reserve: workgroup slots a scan launch leaves free (until changed)
    bool have_matrix = false;
    int8_t* d_query = nullptr;
    size_t query_capacity = 0;
    // sw_set_query stages the query through a small ring of pinned host buffers, so that the upload needs no host
    // synchronisation (the caller's buffer is free again when the call returns, the copy runs stream-ordered)
    static constexpr int kQuerySlots = 4;
    int8_t* h_query[kQuerySlots] = {};
    size_t h_query_capacity[kQuerySlots] = {};
    hipEvent_t query_copied[kQuerySlots] = {};
    bool query_slot_used[kQuerySlots] = {};
    int query_next = 0;
    // sw_set_query_pssm: the query is a position-specific scoring matrix, staged on the device in the tiled form of
    // sw_pssm.hpp; d_query and the matrix are not read while it is installed
    bool pssm_mode = false;
    int8_t* d_pssm = nullptr;
    size_t pssm_capacity = 0;
    int pssm_max = 1;            // largest entry of the installed PSSM: what matrix_max is to a letter query
    swi::Profile profiles[4][4][3];  // [kind][shape: 0 = 16-lane groups, 1 = 64-lane groups, 2 = 8-lane groups, 3 = 4-lane groups][plain | column frame | uniform frame]
    int64_t long16_min_default = -1;  // the built-in rule (sw_set_long16_min(ctx, -1) returns to it)
    int matrix_max = 1;          // largest substitution score of the installed matrix
    bool check_bounds = false;   // CUDASW4_AMD_CHECK_BOUNDS=1 (debug): every scan first verifies the max_subject_len contract on the device (synchronises)
    uint32_t pipe_spin_limit = 1u << 20;  // CUDASW4_AMD_PIPE_SPIN_LIMIT: polls (~2 us each) before a pipeline stage gives up waiting
    int32_t pipe_drop_stage = -1;         // CUDASW4_AMD_PIPE_TEST_DROP_STAGE (tests): this stage of every subject is lost
    int32_t pipe_cpl = 0;                 // CUDASW4_AMD_PIPE_CPL=4|8|16: columns per lane of a stage (0: by the subjects' length)
    int32_t pipe_quorum = 0;              // (0: all tickets)
    int32_t pipe_slot = 0;                // sw_set_rows_pipeline_slot: VGPRs a stage occupies (128 / 168 / 256; 0: what it needs)
};
