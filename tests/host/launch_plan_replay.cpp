// launch_plan_replay.cpp — tests/test_launch_plan_cpu.py: the launch plan (cudasw4_amd/csrc/sw_plan.hpp) without a context
// and without a device.  Links libcudasw4_amd.so, calls swp::plan_launch over the grid given on the command line and
//   * writes what the public planning calls would answer, as int64 words in grid order, to stdout (the test compares them
//     with the recorded table), and
//   * checks that sizing agrees with launching (properties (a), (b), (c) below); violations go to stderr, their number
//     is the exit status (capped at 100).
// The tuning comes from the environment (swp::settings_from_env), as in sw_ctx_create.
// usage: launch_plan_replay NUM_CUS SCORE_MAXES QLENS PARTS NS MAX_SUBJECT_LENS GAPS(gop:gex,...) SERVICE_WORKGROUPS
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "sw_plan.hpp"

using swp::LaunchPlan;
using swp::LaunchRequest;
using swp::PlanSettings;

namespace {
constexpr int kNumPartitions = 36;   // SW_NUM_LENGTH_PARTITIONS
bool packed(int kind) { return kind == 0 || kind == 1; }          // SW_KIND_F16X2, SW_KIND_I16X2
int fallback_kind(int kind) { return kind == 0 ? 3 : 2; }         // ... are served by SW_KIND_F32, SW_KIND_I32

std::vector<long long> list_of(const char* arg) {
    std::vector<long long> v;
    for (const char* p = arg; *p;) {
        char* end = nullptr;
        v.push_back(strtoll(p, &end, 10));
        p = (*end == ',' || *end == ':') ? end + 1 : end;
        if (end == p && *end) break;
    }
    return v;
}

int violations = 0;
void violation(const char* what, const LaunchRequest& r, const PlanSettings& s, const std::string& detail) {
    if (violations++ < 20)
        fprintf(stderr, "%s: kind %d part %d n %d max_len %d qlen %d score_max %d gaps (%d, %d) scratch %zu: %s\n", what, r.kind, r.part_id, r.n,
                r.max_subject_len, s.qlen, s.score_max, r.gop, r.gex, r.scratch, detail.c_str());
}

LaunchRequest sizing(int kind, int part, int n, int max_len) {
    LaunchRequest r;
    r.kind = kind; r.part_id = part; r.n = n; r.max_subject_len = max_len;
    return r;
}
LaunchRequest launching(int kind, int part, int n, int max_len, int gop, int gex, size_t scratch) {
    LaunchRequest r = sizing(kind, part, n, max_len);
    r.gaps_known = true; r.gop = gop; r.gex = gex; r.ovf_list = true; r.scratch = scratch;
    return r;
}

// Sizing agrees with launching.  `need` is what sw_scan_temp_bytes reports for the request.
void check_sizing(const PlanSettings& s, int kind, int part, int n, int max_len, const std::vector<std::pair<int, int>>& gaps) {
    if (part < 0 && packed(kind)) return;   // (a re-score list runs a 32-bit kind: the entry points refuse a packed one)
    const LaunchPlan size_own = swp::plan_launch(s, sizing(kind, part, n, max_len));
    const size_t need = size_own.scratch_needed;
    for (const auto& g : gaps) {
        const LaunchPlan free_plan = swp::plan_launch(s, launching(kind, part, n, max_len, g.first, g.second, swp::kUnlimitedScratch));
        // (a) whatever scratch is offered, the grid's share of it is inside it — or the plan says that not even one workgroup fits
        for (size_t offer : {(size_t)0, size_own.bytes_per_wg, free_plan.bytes_per_wg, need / 2, need}) {
            const LaunchRequest r = launching(kind, part, n, max_len, g.first, g.second, offer);
            const LaunchPlan lp = swp::plan_launch(s, r);
            if (!lp.multi) continue;
            if (lp.scratch_too_small != (offer < lp.bytes_per_wg)) violation("(a) SW_ERR_TEMP condition", r, s, "flag and sizes disagree");
            if (!lp.scratch_too_small && (size_t)lp.grid * lp.bytes_per_wg > offer)
                violation("(a) grid x bytes_per_wg exceeds the offer", r, s, std::to_string(lp.grid) + " x " + std::to_string(lp.bytes_per_wg));
            if (!lp.scratch_too_small && lp.nbatches > 0 && lp.grid < 1) violation("(a) empty grid", r, s, "");
        }
        const LaunchRequest r = launching(kind, part, n, max_len, g.first, g.second, need);
        const LaunchPlan lp = swp::plan_launch(s, r);
        if (g.first == -11 && g.second == -1) {
            // (b) the default gap scores and exactly the reported scratch: no clamp engages, the launch is what was sized
            // (a packed launch that falls back: what was sized for its 32-bit kind)
            const LaunchPlan sized = lp.fell_back ? swp::plan_launch(s, sizing(fallback_kind(kind), part, n, max_len)) : size_own;
            if (lp.kind != sized.kind || lp.lanes != sized.lanes || lp.chain != sized.chain || lp.stream_cols != sized.stream_cols ||
                lp.lcap != sized.lcap || lp.grid != sized.grid || lp.scratch_too_small)
                violation("(b) launch differs from sizing", r, s,
                          "chain " + std::to_string(lp.chain) + "/" + std::to_string(sized.chain) + " cols " + std::to_string(lp.stream_cols) + "/" +
                              std::to_string(sized.stream_cols) + " lcap " + std::to_string(lp.lcap) + "/" + std::to_string(sized.lcap) + " grid " +
                              std::to_string(lp.grid) + "/" + std::to_string(sized.grid));
        } else if (lp.multi && (lp.scratch_too_small || (size_t)lp.grid * lp.bytes_per_wg > need)) {
            // (c) any other gap extension: never more than was given
            violation("(c) launch needs more than was sized", r, s, std::to_string(lp.grid) + " x " + std::to_string(lp.bytes_per_wg));
        }
    }
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 9) {
        fprintf(stderr, "usage: %s NUM_CUS SCORE_MAXES QLENS PARTS NS MAX_SUBJECT_LENS GAPS SERVICE_WORKGROUPS\n", argv[0]);
        return 101;
    }
    PlanSettings s;
    s.num_cus = atoi(argv[1]);
    swp::settings_from_env(s);
    const auto score_maxes = list_of(argv[2]), qlens = list_of(argv[3]), parts = list_of(argv[4]), ns = list_of(argv[5]), lens = list_of(argv[6]),
               gap_words = list_of(argv[7]), service = list_of(argv[8]);
    std::vector<std::pair<int, int>> gaps;
    for (size_t i = 0; i + 1 < gap_words.size(); i += 2) gaps.emplace_back((int)gap_words[i], (int)gap_words[i + 1]);
    std::vector<long long> out, out_service;
    s.have_query = true;
    for (long long score_max : score_maxes)
        for (long long qlen : qlens) {
            s.score_max = (int)score_max;
            s.qlen = (int32_t)qlen;
            for (int kind = 0; kind < 4; kind++) {
                for (long long max_len : lens)
                    for (long long wg : service) {   // sw_rescore_service_temp_bytes
                        LaunchRequest r = sizing(kind, -1, 0, (int)max_len);
                        r.service_workgroups = (int)wg;
                        out_service.push_back((long long)((size_t)wg * swp::plan_launch(s, r).bytes_per_wg));
                    }
                for (long long part : parts)
                    for (long long n : ns)
                        for (long long max_len : lens) {
                            // sw_plan_launch, sw_launch_vgpr_slot, sw_scan_temp_bytes: one sizing plan
                            const LaunchPlan lp = swp::plan_launch(s, sizing(kind, (int)part, (int)n, (int)max_len));
                            long long bits = 0;   // sw_packed_launch_falls_back: a packed range launch, with an overflow list
                            if (packed(kind) && part >= 0 && part < kNumPartitions)
                                for (size_t g = 0; g < gaps.size(); g++)
                                    if (swp::plan_launch(s, launching(kind, (int)part, (int)n, (int)max_len, gaps[g].first, gaps[g].second, swp::kUnlimitedScratch)).fell_back)
                                        bits |= 1ll << g;
                            for (long long v : {(long long)lp.kind, (long long)lp.rows, (long long)lp.nstripes, (long long)lp.lanes, (long long)lp.vgpr_slot,
                                                (long long)lp.scratch_needed, bits})
                                out.push_back(v);
                            check_sizing(s, kind, (int)part, (int)n, (int)max_len, gaps);
                        }
            }
        }
    fwrite(out.data(), sizeof(long long), out.size(), stdout);
    fwrite(out_service.data(), sizeof(long long), out_service.size(), stdout);
    if (violations) fprintf(stderr, "%d violations\n", violations);
    return std::min(violations, 100);
}
