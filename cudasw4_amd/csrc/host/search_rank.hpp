// search_rank.hpp — ranking by E-value (an extension): the host arithmetic — the Z-score an E-value
// threshold stands for, the double-precision order of a few candidates — and the hooks that make SearchDriver rank with
// sw_zscore_keys and sw_gather_hits (include/cudasw4_amd_rank.h).
//
// Kept out of search_driver.cpp and driver_capi.cpp like search_stats.cpp: tests/host/fake_gpu links exactly those files
// against a fake of the C ABI that has neither kernel.
#pragma once
#include <cstdint>

#include "search_driver.hpp"
#include "search_stats.hpp"

namespace swh {

// z_min(X) = -(ln(-ln1p(-X / N)) + gamma) sqrt(6) / pi: the Z-score at which E = N P(z) of DESIGN.md §12 equals X, for
// 0 < X < N.  X >= N: -infinity (every subject passes); X <= 0: +infinity (none does); N <= 0 or a NaN: NaN.
double zscore_for_evalue(int64_t N, double evalue);

// out[0 .. n): the indices 0 .. n-1 by Z-score (hit_statistics: double precision) descending, equal Z-scores by ascending id.
// Without a fit: by raw score descending, then ascending id — the order of a score-ranked list.
void rank_order(const SearchStats& stats, const int32_t* scores, const int32_t* lengths, const int64_t* ids, int n, int32_t* out);

// byEvalue: switch the statistics on (enable_statistics) and rank every query submitted from now on by E-value; maxEvalue > 0
// also counts the subjects with E <= maxEvalue (ScanResult::significant).  !byEvalue: rank by raw score again (the statistics
// stay as they are).  Not with queries in flight.
void set_ranking(SearchDriver& driver, bool byEvalue, double maxEvalue);

}  // namespace swh
