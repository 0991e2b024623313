// shuffle_stats.cpp — ShuffleCalibrator, the sample / replica / permutation rules and the C entry points
// swdrv_calibrate_shuffled / swdrv_calibrate_shuffled_pssm / swdrv_shuffle_sample / swdrv_shuffle_replicas /
// swdrv_shuffle_permutation / swdrv_set_rank_fit.
#include "shuffle_stats.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

namespace swh {

// ---- the definition: pure host code (a host-only build — under a sanitizer — compiles this part alone) ----

namespace {
inline uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}
}  // namespace

std::vector<int64_t> shuffle_sample(int64_t n, int64_t maxSubjects) {
    if (n < 0 || maxSubjects < 1) throw std::runtime_error("shuffle sample: n must not be negative and maxSubjects at least 1");
    const int64_t m = std::min(n, maxSubjects);
    std::vector<int64_t> ids(static_cast<size_t>(m));
    // (2 j + 1) n < 2 M n: 128-bit products keep any int64 n exact
    for (int64_t j = 0; j < m; j++) ids[size_t(j)] = int64_t((static_cast<unsigned __int128>(2 * j + 1) * static_cast<unsigned __int128>(n)) / static_cast<unsigned __int128>(2 * m));
    return ids;
}

int32_t shuffle_replicas(int64_t M, int32_t shuffles) {
    if (shuffles < 0 || shuffles > kShuffleMaxReplicas) throw std::runtime_error("shuffles must lie in [1, " + std::to_string(kShuffleMaxReplicas) + "]");
    if (shuffles > 0) return shuffles;
    const int64_t m = std::max<int64_t>(M, 1);
    return int32_t(std::min<int64_t>(kShuffleMaxReplicas, std::max<int64_t>(1, (kShuffleTargetScores + m - 1) / m)));
}

void shuffle_permutation(int32_t L, uint32_t seed, int64_t id, uint32_t replica, int32_t* out) {
    if (L <= 0) return;
    if (!out) throw std::runtime_error("shuffle permutation: null output");
    if (L == 1) { out[0] = 0; return; }
    const uint64_t u = uint64_t(id);
    const uint32_t k = mix32(mix32(mix32(mix32(seed) ^ uint32_t(u)) ^ uint32_t(u >> 32)) ^ replica);
    int bits = 0;
    for (uint32_t v = uint32_t(L) - 1; v; v >>= 1) bits++;
    const int h = std::max(1, (bits + 1) / 2);
    const uint32_t mask = (uint32_t(1) << h) - 1;
    for (int32_t i = 0; i < L; i++) {
        uint32_t c = uint32_t(i);
        do {
            uint32_t l = c >> h, r = c & mask;
            for (uint32_t rd = 0; rd < 4; rd++) {
                const uint32_t f = mix32(r ^ k ^ (rd * 0x9e3779b9u)) & mask;
                const uint32_t t = l ^ f;
                l = r;
                r = t;
            }
            c = (l << h) | r;
        } while (c >= uint32_t(L));
        out[i] = int32_t(c);
    }
}

}  // namespace swh

#ifndef SWH_STATS_HOST_ONLY
#include "../../../include/cudasw4_amd_pssm.h"
#include "../../../include/cudasw4_amd_shuffle.h"
#include "../../../include/cudasw4_amd_stats.h"

namespace swh {

namespace {

void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string("shuffled statistics: ") + what + ": " + hipGetErrorString(e));
}

void sw_check(int rc, const char* what) {
    if (rc != SW_OK) throw std::runtime_error(std::string("shuffled statistics: ") + what + ": " + sw_last_error());
}

size_t round_up(size_t x) { return (x + 255) / 256 * 256; }

template <class T>
T* device_alloc(size_t count) {
    void* p = nullptr;
    hip_check(hipMalloc(&p, std::max<size_t>(count * sizeof(T), 256)), "hipMalloc");
    return static_cast<T*>(p);
}

}  // namespace

ShuffleCalibrator::ShuffleCalibrator(const SearchDriver& driver, int32_t maxSubjects, int32_t shuffles, uint32_t seed)
    : d_(driver), seed_(seed) {
    if (maxSubjects < 1) throw std::runtime_error("shuffled statistics: the sample must hold at least one subject");
    const int64_t n = int64_t(driver.numSequences());
    if (n == 0) throw std::runtime_error("shuffled statistics: no database");
    ids_ = shuffle_sample(n, maxSubjects);
    replicas_ = shuffle_replicas(int64_t(ids_.size()), shuffles);
    const size_t M = ids_.size();

    // the sample in dbdata layout, from the host copy of the DB
    std::vector<int8_t> chars;
    std::vector<uint64_t> offsets(M + 1, 0);
    lengths_.resize(M);
    for (size_t j = 0; j < M; j++) {
        const std::string s = driver.getReferenceSequence(ids_[j] + driver.idBase());
        lengths_[j] = int32_t(s.size());
        const size_t padded = (s.size() + 3) / 4 * 4;
        chars.resize(size_t(offsets[j]) + padded, kOtherCode);
        for (size_t k = 0; k < s.size(); k++) chars[size_t(offsets[j]) + k] = encode_residue(s[k]);
        // the scans the fit stands for read masked subjects: so does the calibration
        if (driver.masksSubjects()) mask_subject(chars.data() + offsets[j], lengths_[j], driver.maskParams(), chars.data() + offsets[j]);
        offsets[j + 1] = offsets[j] + padded;
    }
    blockBytes_ = chars.size();
    stride_ = round_up(blockBytes_);
    // replicas per chunk: what --maxTempBytes holds, one at least
    const size_t fit = std::max<size_t>(d_.memoryConfig().maxTempBytes / std::max<size_t>(stride_, 1), 1);
    chunk_ = int32_t(std::min<size_t>(size_t(replicas_), fit));

    // the launches of one replica: the sample ascends by length like the DB; the long partitions keep launches of their own
    // (wave-wide groups: plan_launch_runs' shapes), the rest is one bulk launch
    {
        const int32_t m = int32_t(M);
        const int32_t i1 = int32_t(std::upper_bound(lengths_.begin(), lengths_.end(), 1280) - lengths_.begin());
        const int32_t i2 = int32_t(std::upper_bound(lengths_.begin(), lengths_.end(), 8000) - lengths_.begin());
        const bool merge = size_t(i2 - i1) >= kLongPartitionMergeMin;
        const int32_t bulkEnd = merge ? i2 : i1;
        if (i2 < m) ranges_.push_back(Range{kNumLengthPartitions - 1, i2, m, lengths_[size_t(m) - 1]});
        if (!merge && i1 < i2) ranges_.push_back(Range{kNumLengthPartitions - 2, i1, i2, lengths_[size_t(i2) - 1]});
        if (bulkEnd > 0) ranges_.push_back(Range{kNumLengthPartitions - 3, 0, bulkEnd, lengths_[size_t(bulkEnd) - 1]});
    }

    device_ = driver.deviceOf(0);
    sw_check(sw_ctx_create(device_, &ctx_), "sw_ctx_create");
    try {
        sw_check(sw_set_matrix(ctx_, driver.matrix().m.data(), driver.matrix().dim), "sw_set_matrix");
        hip_check(hipSetDevice(device_), "hipSetDevice");
        hip_check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
        chars_ = device_alloc<int8_t>(chars.size());
        offsets_ = device_alloc<uint64_t>(M + 1);
        keys_ = device_alloc<int64_t>(M);
        lengthsDev_ = device_alloc<int32_t>(M * size_t(chunk_));
        shuffled_ = device_alloc<int8_t>(stride_ * size_t(chunk_));
        scores_ = device_alloc<float>(M * size_t(chunk_));
        scoreIds_ = device_alloc<int32_t>(M * size_t(chunk_));
        table_ = device_alloc<ScoreTable>(1);
        std::vector<int32_t> repeated(M * size_t(chunk_));
        for (int32_t r = 0; r < chunk_; r++) std::copy(lengths_.begin(), lengths_.end(), repeated.begin() + size_t(r) * M);
        if (!chars.empty()) hip_check(hipMemcpy(chars_, chars.data(), chars.size(), hipMemcpyHostToDevice), "hipMemcpy");
        hip_check(hipMemcpy(offsets_, offsets.data(), offsets.size() * sizeof(uint64_t), hipMemcpyHostToDevice), "hipMemcpy");
        hip_check(hipMemcpy(keys_, ids_.data(), M * sizeof(int64_t), hipMemcpyHostToDevice), "hipMemcpy");
        hip_check(hipMemcpy(lengthsDev_, repeated.data(), repeated.size() * sizeof(int32_t), hipMemcpyHostToDevice), "hipMemcpy");
    } catch (...) {
        release();
        throw;
    }
}

void ShuffleCalibrator::release() {
    if (hipSetDevice(device_) == hipSuccess) {
        if (stream_) (void)hipStreamSynchronize(stream_);
        void* bufs[] = {chars_, offsets_, keys_, lengthsDev_, shuffled_, scores_, scoreIds_, table_, temp_};
        for (void* p : bufs)
            if (p) (void)hipFree(p);
        if (stream_) (void)hipStreamDestroy(stream_);
    }
    if (ctx_) sw_ctx_destroy(ctx_);
    ctx_ = nullptr;
    stream_ = nullptr;
}

ShuffleCalibrator::~ShuffleCalibrator() { release(); }

std::unique_ptr<Calibration> ShuffleCalibrator::calibrate(const char* query, int32_t qlen) {
    if (qlen <= 0 || !query) throw std::runtime_error("shuffled statistics: empty query");
    const SubstitutionMatrix& m = d_.matrix();
    std::vector<int8_t> q(static_cast<size_t>(qlen));
    for (int32_t i = 0; i < qlen; i++) q[size_t(i)] = m.dim == 25 ? encode_residue25(query[i]) : encode_residue(query[i]);
    hip_check(hipSetDevice(device_), "hipSetDevice");
    sw_check(sw_set_query(ctx_, q.data(), qlen, stream_), "sw_set_query");
    return run();
}

std::unique_ptr<Calibration> ShuffleCalibrator::calibrate(const int8_t* pssm, int32_t qlen) {
    if (qlen <= 0 || !pssm) throw std::runtime_error("shuffled statistics: empty PSSM");
    if (qlen > SW_PSSM_MAX_QUERY_LEN) throw std::runtime_error("shuffled statistics: PSSM too long");
    for (int32_t i = 0; i < qlen; i++)
        if (pssm[size_t(i) * SW_PSSM_COLUMNS + 20] >= 0)
            throw std::runtime_error("shuffled statistics: PSSM row " + std::to_string(i) + ": column 20 (other / padding) must be negative");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    sw_check(sw_set_query_pssm(ctx_, pssm, qlen, stream_), "sw_set_query_pssm");
    return run();
}

// the query is installed: shuffle, scan and histogram the replicas chunk by chunk, then fit
std::unique_ptr<Calibration> ShuffleCalibrator::run() {
    const int32_t M = int32_t(ids_.size());
    constexpr int kKind = SW_KIND_I32;   // exact for any length (served from fp32 lanes where that is proven exact)
    size_t need = 0;
    for (const Range& g : ranges_) need = std::max(need, sw_scan_temp_bytes(ctx_, kKind, g.part, g.end - g.begin, g.maxLen));
    if (need > tempBytes_) {
        hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        if (temp_) hip_check(hipFree(temp_), "hipFree");
        temp_ = nullptr;
        tempBytes_ = 0;
        hip_check(hipMalloc(&temp_, need), "hipMalloc");
        tempBytes_ = need;
    }
    hip_check(hipMemsetAsync(table_, 0, sizeof(ScoreTable), stream_), "hipMemsetAsync");
    for (int32_t first = 0; first < replicas_; first += chunk_) {
        const int32_t count = std::min(chunk_, replicas_ - first);
        if (blockBytes_)
            sw_check(sw_shuffle_subjects(ctx_, chars_, offsets_, lengthsDev_, keys_, M, seed_, first, count, shuffled_, stride_, stream_),
                     "sw_shuffle_subjects");
        for (int32_t r = 0; r < count; r++)
            for (const Range& g : ranges_)
                sw_check(sw_scan_partition(ctx_, kKind, g.part, shuffled_ + size_t(r) * stride_, offsets_, lengthsDev_, g.begin, g.end - g.begin,
                                           g.maxLen, d_.gapOpen(), d_.gapExtend(), scores_ + size_t(r) * size_t(M), scoreIds_ + size_t(r) * size_t(M),
                                           0, nullptr, nullptr, 0, temp_, tempBytes_, stream_),
                         "sw_scan_partition");
        sw_check(sw_score_histogram(ctx_, scores_, lengthsDev_, int64_t(count) * M, table_->hist, table_->sumlen, &table_->skipped, stream_),
                 "sw_score_histogram");   // (addresses only: table_ is a device pointer)
    }
    std::unique_ptr<Calibration> out(new Calibration);
    hip_check(hipMemcpyAsync(&out->table, table_, sizeof(ScoreTable), hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync");
    hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    if (out->table.skipped) throw std::runtime_error("shuffled statistics: internal error (a shuffled subject was not scored)");
    out->stats = stats_from_table(out->table);
    out->subjects = M;
    out->replicas = replicas_;
    return out;
}

}  // namespace swh
#endif   // SWH_STATS_HOST_ONLY

#ifdef SWH_DRIVER_CAPI   // libcudasw4_host.so (with driver_capi.cpp); `align` links the code above alone
#include "../../../include/cudasw4_amd_driver.h"
#include "driver_handle.hpp"

namespace {
template <class F>
int guarded_shuffle(F&& f) {
    try {
        return f();
    } catch (const std::exception& e) {
        swh::set_driver_error(e.what());
        return -1;
    }
}

// query != nullptr: the letter form; else the PSSM form
int calibrate_capi(swdrv* d, const char* query, const int8_t* pssm, int32_t qlen, int32_t max_subjects, int32_t shuffles, uint32_t seed,
                   swdrv_stats* out, uint32_t* hist, uint64_t* sumlen, int32_t* subjects, int32_t* replicas) {
    return guarded_shuffle([&] {
        if (!d || !d->driver) throw std::runtime_error("null driver");
        if (!query && !pssm) throw std::runtime_error("shuffled statistics: null query");
        // the sample of (DB, M, R, seed) stays on the device between calls
        swdrv::CalibratorKey key{d->db.get(), max_subjects, shuffles, seed};
        if (!d->calibrator || !(d->calibratorKey == key)) {
            d->calibrator.reset();
            d->calibrator = std::make_shared<swh::ShuffleCalibrator>(*d->driver, max_subjects, shuffles, seed);
            d->calibratorKey = key;
        }
        const std::unique_ptr<swh::Calibration> c = query ? d->calibrator->calibrate(query, qlen) : d->calibrator->calibrate(pssm, qlen);
        if (out) {
            out->a = c->stats.a; out->b1 = c->stats.b1; out->sd = c->stats.sd;
            out->n_included = c->stats.nIncluded; out->N = c->stats.N; out->rounds = c->stats.rounds; out->status = int32_t(c->stats.status);
        }
        if (hist) std::memcpy(hist, c->table.hist, sizeof c->table.hist);
        if (sumlen) std::memcpy(sumlen, c->table.sumlen, sizeof c->table.sumlen);
        if (subjects) *subjects = c->subjects;
        if (replicas) *replicas = c->replicas;
        return 0;
    });
}
}  // namespace

extern "C" int swdrv_calibrate_shuffled(swdrv* d, const char* query, int32_t qlen, int32_t max_subjects, int32_t shuffles, uint32_t seed,
                                        swdrv_stats* out, uint32_t* hist, uint64_t* sumlen, int32_t* subjects, int32_t* replicas) {
    if (!query) {
        swh::set_driver_error("shuffled statistics: null query");
        return -1;
    }
    return calibrate_capi(d, query, nullptr, qlen, max_subjects, shuffles, seed, out, hist, sumlen, subjects, replicas);
}

extern "C" int swdrv_calibrate_shuffled_pssm(swdrv* d, const int8_t* pssm, int32_t qlen, int32_t max_subjects, int32_t shuffles,
                                             uint32_t seed, swdrv_stats* out, uint32_t* hist, uint64_t* sumlen, int32_t* subjects,
                                             int32_t* replicas) {
    if (!pssm) {
        swh::set_driver_error("shuffled statistics: null PSSM");
        return -1;
    }
    return calibrate_capi(d, nullptr, pssm, qlen, max_subjects, shuffles, seed, out, hist, sumlen, subjects, replicas);
}

extern "C" int swdrv_set_rank_fit(swdrv* d, const swdrv_stats* fit) {
    return guarded_shuffle([&] {
        if (!d || !d->driver) throw std::runtime_error("null driver");
        if (!fit) {
            d->driver->setRankFit(nullptr);
            return 0;
        }
        swh::RankFit f;
        f.ok = fit->status == SWDRV_STATS_OK; f.a = fit->a; f.b1 = fit->b1; f.sd = fit->sd;
        d->driver->setRankFit(&f);
        return 0;
    });
}

extern "C" int swdrv_shuffle_sample(int64_t n, int64_t max_subjects, int64_t* out_ids) {
    return guarded_shuffle([&] {
        if (std::min(n, max_subjects) > int64_t(INT32_MAX)) throw std::runtime_error("shuffle sample: more than 2^31 - 1 subjects");
        const std::vector<int64_t> ids = swh::shuffle_sample(n, max_subjects);
        if (out_ids) std::copy(ids.begin(), ids.end(), out_ids);
        return int(ids.size());
    });
}

extern "C" int swdrv_shuffle_replicas(int64_t M, int32_t shuffles) {
    return guarded_shuffle([&] {
        if (M < 0) throw std::runtime_error("shuffle replicas: M must not be negative");
        return int(swh::shuffle_replicas(M, shuffles));
    });
}

extern "C" int swdrv_shuffle_permutation(int32_t L, uint32_t seed, int64_t id, int32_t replica, int32_t* out) {
    return guarded_shuffle([&] {
        if (replica < 0) throw std::runtime_error("shuffle permutation: the replica must not be negative");
        swh::shuffle_permutation(L, seed, id, uint32_t(replica), out);
        return 0;
    });
}
#endif
