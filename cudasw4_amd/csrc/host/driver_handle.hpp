// driver_handle.hpp — the object behind swdrv* (include/cudasw4_amd_driver.h), shared by the files that implement that
// C ABI: driver_capi.cpp and hit_alignment.cpp.
#pragma once
#include <memory>
#include <string>

#include "db_format.hpp"
#include "search_driver.hpp"

namespace swh {
class ShuffleCalibrator;   // shuffle_stats.hpp
}

struct swdrv {
    std::unique_ptr<swh::SearchDriver> driver;
    std::shared_ptr<swh::Database> db;
    int lastRescored = 0;
    std::vector<swh::ScoreTable> lastTable;   // ScanResult::table of the query collected last (search_stats.cpp)
    int64_t lastSignificant = -1;             // ScanResult::significant and ::zMin of that query (search_rank.cpp)
    double lastZMin = 0;
    // the calibrator of swdrv_calibrate_shuffled (shuffle_stats.cpp) and what it was made for: its sample stays on the device
    // between calls.  (Declared behind `driver`: destroyed before it.)
    struct CalibratorKey {
        const void* db = nullptr;
        int32_t maxSubjects = 0, shuffles = 0;
        uint32_t seed = 0;
        bool operator==(const CalibratorKey& o) const { return db == o.db && maxSubjects == o.maxSubjects && shuffles == o.shuffles && seed == o.seed; }
    };
    std::shared_ptr<swh::ShuffleCalibrator> calibrator;
    CalibratorKey calibratorKey;
};

namespace swh {
// the text swdrv_last_error() returns on this thread (driver_capi.cpp)
void set_driver_error(const std::string& text);
}  // namespace swh
