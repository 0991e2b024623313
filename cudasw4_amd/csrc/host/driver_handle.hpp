// driver_handle.hpp — the object behind swdrv* (include/cudasw4_amd_driver.h), shared by the files that implement that
// C ABI: driver_capi.cpp and hit_alignment.cpp.
#pragma once
#include <memory>
#include <string>

#include "db_format.hpp"
#include "search_driver.hpp"

struct swdrv {
    std::unique_ptr<swh::SearchDriver> driver;
    std::shared_ptr<swh::Database> db;
    int lastRescored = 0;
    std::vector<swh::ScoreTable> lastTable;   // ScanResult::table of the query collected last (search_stats.cpp)
    int64_t lastSignificant = -1;             // ScanResult::significant and ::zMin of that query (search_rank.cpp)
    double lastZMin = 0;
};

namespace swh {
// the text swdrv_last_error() returns on this thread (driver_capi.cpp)
void set_driver_error(const std::string& text);
}  // namespace swh
