// search_rank.cpp — ranking by E-value: the threshold's Z-score, the host merge, the driver's hooks and the C entry points
// swdrv_set_ranking / swdrv_last_ranking / swdrv_zscore_for_evalue / swdrv_rank_order.
#include "search_rank.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <numeric>
#include <stdexcept>
#include <vector>

#ifndef SWH_STATS_HOST_ONLY   // (a host-only build — the arithmetic under a sanitizer — leaves the kernel library out)
#include "../../../include/cudasw4_amd_rank.h"
#endif

namespace swh {

namespace {
constexpr double kEulerGamma = 0.5772156649015329;
}  // namespace

double zscore_for_evalue(int64_t N, double evalue) {
    if (N <= 0 || std::isnan(evalue)) return std::numeric_limits<double>::quiet_NaN();
    if (evalue <= 0.0) return std::numeric_limits<double>::infinity();
    if (evalue >= double(N)) return -std::numeric_limits<double>::infinity();
    return -(std::log(-std::log1p(-evalue / double(N))) + kEulerGamma) * std::sqrt(6.0) / M_PI;
}

void rank_order(const SearchStats& stats, const int32_t* scores, const int32_t* lengths, const int64_t* ids, int n, int32_t* out) {
    if (n < 0 || (n > 0 && (!scores || !lengths || !ids || !out))) throw std::runtime_error("rank_order: bad arguments");
    std::vector<double> z(size_t(n), 0.0);
    for (int i = 0; i < n; i++) z[size_t(i)] = stats.fitted() ? hit_statistics(stats, scores[i], lengths[i]).z : double(scores[i]);
    std::iota(out, out + n, int32_t(0));
    std::sort(out, out + n, [&](int32_t x, int32_t y) {
        if (z[size_t(x)] != z[size_t(y)]) return z[size_t(x)] > z[size_t(y)];
        if (ids[x] != ids[y]) return ids[x] < ids[y];
        return x < y;
    });
}

#ifndef SWH_STATS_HOST_ONLY
namespace {
SearchStats stats_of(const RankFit& f) {
    SearchStats s;
    s.a = f.a; s.b1 = f.b1; s.sd = f.sd; s.N = f.N;
    s.status = f.ok ? StatsStatus::Ok : StatsStatus::NoFit;
    return s;
}
RankFit fit_hook(const ScoreTable& table) {
    const SearchStats s = stats_from_table(table);
    RankFit f;
    f.ok = s.fitted(); f.a = s.a; f.b1 = s.b1; f.sd = s.sd; f.N = s.N;
    return f;
}
void order_hook(const RankFit& fit, const int32_t* scores, const int32_t* lengths, const int64_t* ids, int n, int32_t* out) {
    rank_order(stats_of(fit), scores, lengths, ids, n, out);
}
const RankHooks kHooks = {&sw_zscore_keys, &sw_gather_hits, &fit_hook, &zscore_for_evalue, &order_hook};
}  // namespace

void set_ranking(SearchDriver& driver, bool byEvalue, double maxEvalue) {
    if (!byEvalue) { driver.setRanking(nullptr, 0); return; }
    if (std::isnan(maxEvalue)) throw std::runtime_error("set_ranking: the E-value threshold is not a number");
    enable_statistics(driver, true);
    driver.setRanking(&kHooks, maxEvalue);
}
#endif

}  // namespace swh

#ifdef SWH_DRIVER_CAPI   // libcudasw4_host.so (with driver_capi.cpp); `align` links the functions above alone
#include "../../../include/cudasw4_amd_driver.h"
#include "driver_handle.hpp"

namespace {
template <class F>
int guarded_rank(F&& f) {
    try {
        f();
        return 0;
    } catch (const std::exception& e) {
        swh::set_driver_error(e.what());
        return -1;
    }
}
}  // namespace

extern "C" int swdrv_set_ranking(swdrv* d, int mode, double max_evalue) {
    return guarded_rank([&] {
        if (!d || !d->driver) throw std::runtime_error("null driver");
        if (mode != SWDRV_RANK_SCORE && mode != SWDRV_RANK_EVALUE) throw std::runtime_error("unknown ranking mode");
        swh::set_ranking(*d->driver, mode == SWDRV_RANK_EVALUE, max_evalue);
    });
}

extern "C" int swdrv_last_ranking(swdrv* d, int64_t* count, double* z_min) {
    return guarded_rank([&] {
        if (!d || !d->driver) throw std::runtime_error("null driver");
        if (count) *count = d->lastSignificant;
        if (z_min) *z_min = d->lastZMin;
    });
}

extern "C" double swdrv_zscore_for_evalue(int64_t N, double evalue) { return swh::zscore_for_evalue(N, evalue); }

extern "C" int swdrv_rank_order(const swdrv_stats* stats, const int32_t* scores, const int32_t* lengths, const int64_t* ids, int n,
                                int32_t* out_order) {
    return guarded_rank([&] {
        if (!stats) throw std::runtime_error("bad arguments");
        swh::SearchStats s;
        s.a = stats->a; s.b1 = stats->b1; s.sd = stats->sd; s.nIncluded = stats->n_included; s.N = stats->N; s.rounds = stats->rounds;
        s.status = stats->status == SWDRV_STATS_OK ? swh::StatsStatus::Ok : swh::StatsStatus::NoFit;
        swh::rank_order(s, scores, lengths, ids, n, out_order);
    });
}
#endif
