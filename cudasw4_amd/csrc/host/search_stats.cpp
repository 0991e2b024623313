// search_stats.cpp — search statistics: the fit, the per-hit conversion, the score tap and the C entry points
// swdrv_set_statistics / swdrv_last_statistics / swdrv_stats_from_histogram / swdrv_evalues / swdrv_length_bin.
#include "search_stats.hpp"

#include <cmath>
#include <cstring>
#include <stdexcept>

#ifndef SWH_STATS_HOST_ONLY   // (a host-only build — the fit under a sanitizer — leaves the kernel library out)
#include "../../../include/cudasw4_amd_stats.h"
static_assert(swh::kStatsLengthBins == SW_STATS_LBINS && swh::kStatsScoreBins == SW_STATS_SBINS, "ScoreTable is the library's table");
#endif

namespace swh {

namespace {
constexpr int kL = kStatsLengthBins, kS = kStatsScoreBins;
constexpr int kMaxRounds = 10;
constexpr int64_t kMinIncluded = 100;
constexpr double kZCut = 5.0;
constexpr double kEulerGamma = 0.5772156649015329;
}  // namespace

int stats_length_bin(int32_t length) {
    if (length <= 1) return 0;
    const int e = 31 - __builtin_clz(uint32_t(length));
    return 2 * e + ((length >> (e - 1)) & 1);
}

SearchStats stats_from_histogram(const uint32_t* hist, const uint64_t* sumlen) {
    if (!hist || !sumlen) throw std::runtime_error("statistics: null table");
    SearchStats st;
    double x[kL];
    bool populated[kL];
    for (int b = 0; b < kL; b++) {
        uint64_t nb = 0;
        for (int s = 0; s < kS; s++) nb += hist[b * kS + s];
        st.N += int64_t(nb);
        populated[b] = nb > 0;
        x[b] = populated[b] ? std::log(double(sumlen[b]) / double(nb)) : 0.0;
    }
    // the cells of the current regression: eligible ones to begin with
    std::vector<uint8_t> included(size_t(kL) * kS, 0), next(size_t(kL) * kS, 0);
    for (int b = 0; b < kL; b++)
        for (int s = 1; s <= kS - 2; s++) included[size_t(b) * kS + s] = populated[b];
    for (int round = 1; round <= kMaxRounds; round++) {
        double n = 0, sx = 0, ss = 0, sxx = 0, sxs = 0;
        int64_t count = 0;
        int bins = 0;
        for (int b = 0; b < kL; b++) {
            bool any = false;
            for (int s = 1; s <= kS - 2; s++) {
                if (!included[size_t(b) * kS + s]) continue;
                const double w = double(hist[b * kS + s]);
                any = true;
                count += int64_t(hist[b * kS + s]);
                n += w; sx += w * x[b]; ss += w * double(s); sxx += w * x[b] * x[b]; sxs += w * x[b] * double(s);
            }
            if (any) bins++;
        }
        st.rounds = round;
        st.nIncluded = count;
        if (count < kMinIncluded) { st.status = StatsStatus::NoFit; return st; }
        const double den = n * sxx - sx * sx;
        const double b1 = (den == 0.0 || bins < 2) ? 0.0 : (n * sxs - sx * ss) / den;
        const double a = (ss - b1 * sx) / n;
        double sq = 0;
        for (int b = 0; b < kL; b++)
            for (int s = 1; s <= kS - 2; s++) {
                if (!included[size_t(b) * kS + s]) continue;
                const double r = double(s) - a - b1 * x[b];
                sq += double(hist[b * kS + s]) * r * r;
            }
        const double var = sq / (n - 2.0);
        st.a = a; st.b1 = b1;
        if (!(var > 0.0)) { st.sd = 0; st.status = StatsStatus::NoFit; return st; }
        st.sd = std::sqrt(var);
        st.status = StatsStatus::Ok;
        bool same = true;
        for (int b = 0; b < kL; b++)
            for (int s = 1; s <= kS - 2; s++) {
                const size_t i = size_t(b) * kS + s;
                uint8_t in = 0;
                if (populated[b]) {
                    const double z = (double(s) - a - b1 * x[b]) / st.sd;
                    in = z >= -kZCut && z <= kZCut;
                }
                next[i] = in;
                same = same && in == included[i];
            }
        if (same) break;
        included.swap(next);
    }
    return st;
}

HitStatistics hit_statistics(const SearchStats& s, int32_t score, int32_t length) {
    HitStatistics h;
    if (!s.fitted()) return h;
    h.z = (double(score) - s.a - s.b1 * std::log(double(length < 1 ? 1 : length))) / s.sd;
    const double p = -std::expm1(-std::exp(-(M_PI / std::sqrt(6.0)) * h.z - kEulerGamma));
    h.e = double(s.N) * p;
    return h;
}

#ifndef SWH_STATS_HOST_ONLY
namespace {
int histogram_tap(sw_ctx* ctx, const float* scores, const int32_t* lengths, int64_t n, void* deviceOut, void* stream) {
    auto* t = static_cast<ScoreTable*>(deviceOut);
    return sw_score_histogram(ctx, scores, lengths, n, t->hist, t->sumlen, &t->skipped, stream);   // (addresses only: t is a device pointer)
}
}  // namespace

void enable_statistics(SearchDriver& driver, bool on) { driver.setScoreTap(on ? &histogram_tap : nullptr); }
#endif

}  // namespace swh

#ifdef SWH_DRIVER_CAPI   // libcudasw4_host.so (with driver_capi.cpp); `align` links the functions above alone
#include "../../../include/cudasw4_amd_driver.h"
#include "driver_handle.hpp"

static_assert(SWDRV_STATS_OK == int(swh::StatsStatus::Ok) && SWDRV_STATS_NO_FIT == int(swh::StatsStatus::NoFit), "status codes");

namespace {
void to_c(const swh::SearchStats& s, swdrv_stats* out) {
    out->a = s.a; out->b1 = s.b1; out->sd = s.sd;
    out->n_included = s.nIncluded; out->N = s.N; out->rounds = s.rounds; out->status = int32_t(s.status);
}
template <class F>
int guarded_stats(F&& f) {
    try {
        f();
        return 0;
    } catch (const std::exception& e) {
        swh::set_driver_error(e.what());
        return -1;
    }
}
}  // namespace

extern "C" int swdrv_set_statistics(swdrv* d, int on) {
    return guarded_stats([&] {
        if (!d || !d->driver) throw std::runtime_error("null driver");
        swh::enable_statistics(*d->driver, on != 0);
    });
}

extern "C" int swdrv_last_statistics(swdrv* d, swdrv_stats* out, uint32_t* hist, uint64_t* sumlen) {
    return guarded_stats([&] {
        if (!d || !d->driver) throw std::runtime_error("null driver");
        if (d->lastTable.empty()) throw std::runtime_error("the query collected last was scanned without statistics (swdrv_set_statistics)");
        const swh::ScoreTable& t = d->lastTable.front();
        if (out) to_c(swh::stats_from_table(t), out);
        if (hist) std::memcpy(hist, t.hist, sizeof t.hist);
        if (sumlen) std::memcpy(sumlen, t.sumlen, sizeof t.sumlen);
    });
}

extern "C" int swdrv_stats_from_histogram(const uint32_t* hist, const uint64_t* sumlen, swdrv_stats* out) {
    return guarded_stats([&] {
        if (!out) throw std::runtime_error("null out pointer");
        to_c(swh::stats_from_histogram(hist, sumlen), out);
    });
}

extern "C" int swdrv_evalues(const swdrv_stats* stats, const int32_t* scores, const int32_t* lengths, int n, double* z, double* e) {
    return guarded_stats([&] {
        if (!stats || n < 0 || (n > 0 && (!scores || !lengths))) throw std::runtime_error("bad arguments");
        swh::SearchStats s;
        s.a = stats->a; s.b1 = stats->b1; s.sd = stats->sd; s.nIncluded = stats->n_included; s.N = stats->N; s.rounds = stats->rounds;
        s.status = stats->status == SWDRV_STATS_OK ? swh::StatsStatus::Ok : swh::StatsStatus::NoFit;
        for (int i = 0; i < n; i++) {
            const swh::HitStatistics h = swh::hit_statistics(s, scores[i], lengths[i]);
            if (z) z[i] = h.z;
            if (e) e[i] = h.e;
        }
    });
}

extern "C" int swdrv_length_bin(int32_t length) { return swh::stats_length_bin(length); }
#endif
