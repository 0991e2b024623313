// sw_plan.hpp — the launch plan of a scan: every decision that shapes a launch, made once by plan_launch and read by
// the sizing calls (sw_scan_temp_bytes, sw_rescore_service_temp_bytes), the reporting calls (sw_plan_launch,
// sw_launch_vgpr_slot, sw_packed_launch_falls_back) and the launches themselves.  Declarations only, plain C++ (no HIP
// header): the definitions are sw_api.hip's, and a host program can link the library and call plan_launch without a device.
#pragma once
#include <cstddef>
#include <cstdint>

namespace swp {

// Everything of a context that shapes a launch, and nothing else.
struct PlanSettings {
    // the device
    int num_cus = 0;
    int grid_mult = 4;           // persistent workgroups per CU
    int grid_cap = 0;            // CUDASW4_AMD_GRID_CAP (tests): most workgroups of a scan launch — small DBs then give long claims (sw_stream_kernel.hpp)
    // the installed query
    int32_t qlen = 0;
    bool have_query = false;
    int score_max = 1;           // the largest score one aligned pair of residues can add: the matrix's maximum for a letter query, the PSSM's own for a PSSM query
    // tuning (settings_from_env; sw_set_long16_min)
    bool use_offs = true;        // CUDASW4_AMD_NO_OFFS=1: always the plain recurrence (A/B measurements)
    bool i32_native = false;     // CUDASW4_AMD_I32_NATIVE=1: never compute the int32 kind in fp32 lanes (tests of the int32 kernels)
    int32_t lanes4_max_subject = -1;  // CUDASW4_AMD_LANES4_MAX_SUBJECT: ... when no subject of the launch is longer (-1: 1280)
    int32_t lanes4_max_q = -1;   // CUDASW4_AMD_LANES4_MAX_Q: queries up to this length use 4-lane groups (0: never; -1: the built-in limits)
    int32_t lanes8_max_q = -1;   // CUDASW4_AMD_LANES8_MAX_Q: queries up to this length use 8-lane groups (0: never; -1: the built-in limits)
    int64_t long16_min = -1;     // sw_set_long16_min: partition 34 gets 16-lane groups from this many subjects up (-1: 512)
    int32_t stream_slots = 4;    // CUDASW4_AMD_STREAM=0..16: most batches whose subjects stream through the lanes back to back (sw_stream_kernel.hpp; 0 / 1: sw_scan_kernel, one batch at a time)
    int32_t stream_jump = 0;              // what the zero levels rise by at a slot border (0: 512 for fp16, 2048 for int16)
    int32_t stream_cols_max = 4096;       // most columns of a round of several slots
    int32_t stream_multi_cols_max = 1536; // ... of a multi-stripe query (its border arrays grow with the round)
    int32_t stream_multi_max_subject = -1;    // multi-stripe queries stream subjects up to this length (-1: 320 for fp16, 192 for int16)
    int32_t chain = 3;           // CUDASW4_AMD_CHAIN=1..8: batches a workgroup of the packed multi-stripe sw_scan_kernel claims at once and walks as one virtual subject per stripe (sw_dp_kernel.hpp: "Pair chains"; 1: one batch per claim).  3: the best of the sweep in profiles/pair_chain_results.md
    bool chain_all = false;      // CUDASW4_AMD_CHAIN_ALL=1 (tests): every claim is a chain, also the last rounds of a launch and launches of few batches
};
// the tuning fields as the environment sets them (read now)
void settings_from_env(PlanSettings& s);

constexpr size_t kUnlimitedScratch = ~(size_t)0;

// What a caller asks for.
struct LaunchRequest {
    int kind = 0;
    int part_id = -1;            // the length partition of a plain range; < 0: a re-score list (listed positions)
    int32_t n = 0;               // subjects (of a list: its capacity)
    int32_t max_subject_len = 0;
    // gap scores; not known yet (sizing): the plan assumes an extension of -1 — what the default and almost every caller
    // use; a scratch sized for fewer columns only makes the rounds shorter — and does not ask the fall-back question, but
    // sizes a packed range for the larger of its own need and its 32-bit fall-back's
    bool gaps_known = false;
    int gop = 0, gex = 0;
    bool ovf_list = false;       // an overflow list to flag into (packed kinds cannot run without one)
    // re-score lists (part_id < 0: positions and a count on the device)
    bool claim = false;          // entries are taken by compare-and-swap
    int service_workgroups = 0;  // > 0: a service launch of this many workgroups
    size_t scratch = kUnlimitedScratch;   // the scratch on offer (sizing: unlimited)
};

// Every decision, made once.
struct LaunchPlan {
    bool valid = false;          // false: unknown kind, no query or a negative length — only kind, fell_back, lanes and offs are meaningful
    int kind = 0;                // the kind that runs: int32 in fp32 lanes where that is exact, a packed kind's 32-bit fall-back
    bool fell_back = false;      // a packed launch that cannot run the column-offset recurrence, served by its 32-bit kind
    int lanes = 16, rows = 0, nstripes = 0;
    bool multi = false;
    bool offs = false;           // the column-offset recurrence
    int frame = 0;               // 0 plain recurrence, 1 column frame, 2 uniform frame
    int64_t period = 0;          // frame period K in columns (the uniform frame's is bounded by its level table)
    int64_t flag_period = 0;     // the period the early flags are bounded with
    int stream_slots = 0, stream_cols = 0, stream_room = 0, stream_base = 0, stream_jump = 0;   // after the scratch clamp
    int chain = 1;               // batches per claim, after the scratch clamp
    int32_t lcap = 0;            // border capacity in words per (workgroup, group) array
    int64_t nbatches = 0;
    int grid = 0;                // after the service cap and the scratch clamp
    size_t bytes_per_wg = 0;     // scratch of one workgroup (0: a single stripe needs none)
    size_t scratch_needed = 0;   // what the unclamped plan needs in all
    bool scratch_too_small = false;   // the offer does not hold one workgroup of a multi-stripe plan: SW_ERR_TEMP
    int vgpr_slot = 0;           // VGPRs the kernel occupies (0: no kernel compiled for the plan)
};

LaunchPlan plan_launch(const PlanSettings& s, const LaunchRequest& req);

}  // namespace swp
