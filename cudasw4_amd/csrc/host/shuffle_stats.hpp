// shuffle_stats.hpp — search statistics calibrated on shuffled subjects (an extension): the query is scored
// against a length-stratified sample of the database whose subjects are permuted on the device (sw_shuffle_subjects,
// include/cudasw4_amd_shuffle.h), and the fit of search_stats.hpp is made on THOSE scores.  Permuted subjects keep length and
// composition and are related to nothing, so the fit holds where the scan's own scores do not describe unrelated subjects:
// a database dominated by one family, a database too small to fit, the pseudo database.
//
// Kept out of search_driver.cpp and driver_capi.cpp (like hit_alignment.cpp): tests/host/fake_gpu links exactly those files
// against a fake of the C ABI that has no sw_shuffle_subjects.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../../include/cudasw4_amd.h"
#include "search_driver.hpp"
#include "search_stats.hpp"

namespace swh {

constexpr int32_t kShuffleDefaultSubjects = 10000;
constexpr int32_t kShuffleMaxReplicas = 64;
constexpr int32_t kShuffleTargetScores = 2000;

// ---- the definition (pure host code) ----
// the sampled ids of a database of n sequences: ((2 j + 1) n) / (2 M) for j = 0 .. M - 1, M = min(n, maxSubjects)
std::vector<int64_t> shuffle_sample(int64_t n, int64_t maxSubjects);
// R: `shuffles` when it is given (1 .. 64; 0: not given), else ceil(2000 / M) clamped to [1, 64]
int32_t shuffle_replicas(int64_t M, int32_t shuffles);
// pi of a subject of true length L under (seed, id, replica): out[i] = the position output residue i is taken from
void shuffle_permutation(int32_t L, uint32_t seed, int64_t id, uint32_t replica, int32_t* out);

struct Calibration {
    ScoreTable table;     // of the M x R shuffled subjects
    SearchStats stats;    // its fit (N: the shuffled table's — the statistics of a scan take N from the scan's table)
    int32_t subjects = 0, replicas = 0;
};
// the calibrated statistics of a scan: the calibration's fit with N = the subjects the scan scored
inline SearchStats calibrated_stats(const SearchStats& calibration, int64_t scanN) {
    SearchStats s = calibration;
    s.N = scanN;
    return s;
}
inline int64_t table_count(const ScoreTable& t) {
    int64_t n = 0;
    for (uint32_t c : t.hist) n += int64_t(c);
    return n;
}

// Scores queries against the shuffled sample on the device of the driver's first GPU with a context and a stream of its
// own.  The sample is gathered once from the host copy of the database (resident, streamed, pseudo and array databases
// alike) and stays on the device; it is drawn from the whole database the driver opened, whatever its shard.  The
// calibration depends on the query and the database only: it may run before the scan's collect().
class ShuffleCalibrator {
public:
    // maxSubjects >= 1; shuffles: 1 .. 64, or 0 for the default rule
    ShuffleCalibrator(const SearchDriver& driver, int32_t maxSubjects = kShuffleDefaultSubjects, int32_t shuffles = 0, uint32_t seed = 1);
    ~ShuffleCalibrator();
    ShuffleCalibrator(const ShuffleCalibrator&) = delete;
    ShuffleCalibrator& operator=(const ShuffleCalibrator&) = delete;

    std::unique_ptr<Calibration> calibrate(const char* query, int32_t qlen);      // residue letters, the driver's matrix
    std::unique_ptr<Calibration> calibrate(const int8_t* pssm, int32_t qlen);     // qlen x 21 int8, column 20 negative
    int32_t subjects() const { return int32_t(ids_.size()); }
    int32_t replicas() const { return replicas_; }
    int32_t replicasPerChunk() const { return chunk_; }   // < replicas(): the replicas go through in chunks (--maxTempBytes)

private:
    std::unique_ptr<Calibration> run();   // the query is installed
    void release();
    const SearchDriver& d_;
    int device_ = 0;
    sw_ctx* ctx_ = nullptr;
    hipStream_t stream_ = nullptr;
    uint32_t seed_;
    int32_t replicas_ = 1, chunk_ = 1;
    std::vector<int64_t> ids_;
    std::vector<int32_t> lengths_;
    size_t blockBytes_ = 0, stride_ = 0;
    // the sample on the device, the chunk's replicas, their scores, the table and the scans' scratch
    int8_t* chars_ = nullptr;
    uint64_t* offsets_ = nullptr;
    int32_t* lengthsDev_ = nullptr;   // the sample's lengths, chunk_ times over
    int64_t* keys_ = nullptr;
    int8_t* shuffled_ = nullptr;
    float* scores_ = nullptr;
    int32_t* scoreIds_ = nullptr;
    ScoreTable* table_ = nullptr;
    void* temp_ = nullptr;
    size_t tempBytes_ = 0;
    struct Range { int part; int32_t begin, end, maxLen; };
    std::vector<Range> ranges_;
};

}  // namespace swh
