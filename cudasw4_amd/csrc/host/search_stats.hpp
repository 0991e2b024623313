// search_stats.hpp — search statistics (an extension): Z-scores and E-values by the regression of FASTA /
// SSEARCH (Pearson 1998) on the (length bin, score) histogram a scan leaves (ScoreTable, search_driver.hpp), and the score
// tap that makes SearchDriver fill that table with sw_score_histogram (include/cudasw4_amd_stats.h).
//
// Kept out of search_driver.cpp and driver_capi.cpp (like pssm_query.cpp): tests/host/fake_gpu links exactly those files
// against a fake of the C ABI that has no sw_score_histogram.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "search_driver.hpp"

namespace swh {

enum class StatsStatus : int32_t { Ok = 0, NoFit = 1 };

struct SearchStats {
    double a = 0, b1 = 0, sd = 0;   // an unrelated subject of length L scores a + b1 ln L, residuals of standard deviation sd
    int64_t nIncluded = 0;          // subjects the last regression ran over
    int64_t N = 0;                  // subjects scored
    int32_t rounds = 0;             // regressions computed
    StatsStatus status = StatsStatus::NoFit;
    bool fitted() const { return status == StatsStatus::Ok; }
};

int stats_length_bin(int32_t length);

// the fit of DESIGN.md §12 (pure host code, double precision, sums in ascending (bin, score) order)
SearchStats stats_from_histogram(const uint32_t* hist, const uint64_t* sumlen);
inline SearchStats stats_from_table(const ScoreTable& t) { return stats_from_histogram(t.hist, t.sumlen); }

// z and E of one hit (NoFit: 0 and -1)
struct HitStatistics { double z = 0, e = -1; };
HitStatistics hit_statistics(const SearchStats& s, int32_t score, int32_t length);

// switch the driver's score tap on (sw_score_histogram into a ScoreTable) or off
void enable_statistics(SearchDriver& driver, bool on);

}  // namespace swh
