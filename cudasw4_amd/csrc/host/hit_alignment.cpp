// hit_alignment.cpp — HitAligner, swdrv_align_hits and swdrv_align_hits_pssm: the top hits of a scan aligned with
// sw_align_hits (letter queries) or sw_align_hits_pssm (PSSM queries); swdrv_align_hsps and swdrv_align_hsps_pssm: up to
// max_hsps non-overlapping alignments per hit (sw_align_hsps / sw_align_hsps_pssm).
//
// Kept out of search_driver.cpp and driver_capi.cpp on purpose: tests/host/fake_gpu links exactly those files against a
// fake of the C ABI that has neither.
#include "hit_alignment.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../../include/cudasw4_amd_driver.h"
#include "../../../include/cudasw4_amd_hsps.h"
#include "../../../include/cudasw4_amd_pssm.h"
#include "driver_handle.hpp"
#include "sequence_codec.hpp"

namespace swh {

namespace {

void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string("hit alignment: ") + what + ": " + hipGetErrorString(e));
}

void sw_check(int rc, const char* what) {
    if (rc != SW_OK) throw std::runtime_error(std::string("hit alignment: ") + what + ": " + sw_last_error());
}

size_t round_up(size_t x) { return (x + 255) / 256 * 256; }

// sw_align_args::trace_bytes of a rows x cols rectangle
size_t trace_bytes_for(size_t rows, size_t cols) { return (rows + 511) / 512 * (cols + 63) * 256; }

}  // namespace

std::string cigar_string(const std::vector<uint32_t>& words) {
    if (words.empty()) return "*";
    std::string s;
    for (uint32_t w : words) {
        s += std::to_string(w >> 4);
        switch (w & 15u) {
            case SW_CIGAR_I: s += 'I'; break;
            case SW_CIGAR_D: s += 'D'; break;
            case SW_CIGAR_EQ: s += '='; break;
            default: s += 'X'; break;
        }
    }
    return s;
}

HitAligner::HitAligner(const SearchDriver& driver) : d_(driver) {
    device_ = driver.deviceOf(0);
    sw_check(sw_ctx_create(device_, &ctx_), "sw_ctx_create");
    try {
        sw_check(sw_set_matrix(ctx_, driver.matrix().m.data(), driver.matrix().dim), "sw_set_matrix");
        hip_check(hipSetDevice(device_), "hipSetDevice");
        hip_check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
    } catch (...) {
        sw_ctx_destroy(ctx_);
        throw;
    }
}

HitAligner::~HitAligner() {
    if (hipSetDevice(device_) == hipSuccess) {
        if (stream_) (void)hipStreamSynchronize(stream_);
        for (void* p : buf_)
            if (p) (void)hipFree(p);
        if (stream_) (void)hipStreamDestroy(stream_);
    }
    sw_ctx_destroy(ctx_);
}

void* HitAligner::grow(size_t slot, size_t bytes) {
    bytes = std::max<size_t>(bytes, 256);
    if (cap_[slot] < bytes) {
        if (buf_[slot]) hip_check(hipFree(buf_[slot]), "hipFree");
        buf_[slot] = nullptr;
        cap_[slot] = 0;
        hip_check(hipMalloc(&buf_[slot], bytes), "hipMalloc");
        cap_[slot] = bytes;
    }
    return buf_[slot];
}

std::vector<HitAlignment> HitAligner::align(const char* query, int32_t qlen, const ScanResult& r) {
    return align(query, qlen, r.referenceIds.data(), r.scores.data(), r.scores.size());
}

std::vector<HitAlignment> HitAligner::align(const char* query, int32_t qlen, const int64_t* ids, const int32_t* scores,
                                            size_t n) {
    residentHits_ = 0;
    if (n == 0) return std::vector<HitAlignment>();
    if (qlen <= 0 || !query || !ids || !scores) throw std::runtime_error("hit alignment: empty query or null hit list");
    const std::vector<int8_t> q = encodeQuery(query, qlen);
    return run(q.data(), nullptr, qlen, ids, scores, n);
}

// the query encoded as the scan encoded it
std::vector<int8_t> HitAligner::encodeQuery(const char* query, int32_t qlen) const {
    const SubstitutionMatrix& m = d_.matrix();
    std::vector<int8_t> q(static_cast<size_t>(qlen));
    for (int32_t i = 0; i < qlen; i++) q[size_t(i)] = m.dim == 25 ? encode_residue25(query[i]) : encode_residue(query[i]);
    return q;
}

// the PSSM checked, and its consensus letters as codes (empty: none)
std::vector<int8_t> HitAligner::encodeConsensus(const int8_t* pssm, int32_t qlen, const char* consensus) const {
    for (int32_t i = 0; i < qlen; i++)
        if (pssm[size_t(i) * SW_PSSM_COLUMNS + 20] >= 0)
            throw std::runtime_error("hit alignment: PSSM row " + std::to_string(i) + ": column 20 (other / padding) must be negative");
    std::vector<int8_t> c;
    if (consensus) {
        c.resize(static_cast<size_t>(qlen));
        for (int32_t i = 0; i < qlen; i++) c[size_t(i)] = encode_residue(consensus[i]);
    }
    return c;
}

namespace {

void check_hsp_args(int maxHsps, int minScore) {
    if (maxHsps < 1 || maxHsps > SW_MAX_HSPS)
        throw std::runtime_error("hit alignment: maxHsps must lie in [1, " + std::to_string(SW_MAX_HSPS) + "]");
    if (minScore < 1) throw std::runtime_error("hit alignment: the minimal score of further alignments must be at least 1");
}

// slot 0 of every hit, then its further slots that are SW_ALIGN_OK
HitAligner::HspLists trimmed(std::vector<HitAlignment>&& slots, size_t n, int maxHsps) {
    HitAligner::HspLists out(n);
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < maxHsps; k++) {
            HitAlignment& a = slots[i * size_t(maxHsps) + size_t(k)];
            if (k > 0 && a.r.status != SW_ALIGN_OK) break;
            out[i].push_back(std::move(a));
        }
    return out;
}

}  // namespace

std::vector<HitAlignment> HitAligner::alignSlots(const char* query, int32_t qlen, const int64_t* ids, const int32_t* scores,
                                                 size_t n, int maxHsps, int minScore) {
    check_hsp_args(maxHsps, minScore);
    residentHits_ = 0;
    if (n == 0) return std::vector<HitAlignment>();
    if (qlen <= 0 || !query || !ids || !scores) throw std::runtime_error("hit alignment: empty query or null hit list");
    const std::vector<int8_t> q = encodeQuery(query, qlen);
    return run(q.data(), nullptr, qlen, ids, scores, n, maxHsps, minScore);
}

std::vector<HitAlignment> HitAligner::alignSlots(const int8_t* pssm, int32_t qlen, const char* consensus, const int64_t* ids,
                                                 const int32_t* scores, size_t n, int maxHsps, int minScore) {
    check_hsp_args(maxHsps, minScore);
    residentHits_ = 0;
    if (n == 0) return std::vector<HitAlignment>();
    if (qlen <= 0 || !pssm || !ids || !scores) throw std::runtime_error("hit alignment: empty PSSM or null hit list");
    const std::vector<int8_t> c = encodeConsensus(pssm, qlen, consensus);
    return run(consensus ? c.data() : nullptr, pssm, qlen, ids, scores, n, maxHsps, minScore);
}

HitAligner::HspLists HitAligner::align(const char* query, int32_t qlen, const int64_t* ids, const int32_t* scores, size_t n,
                                       int maxHsps, int minScore) {
    return trimmed(alignSlots(query, qlen, ids, scores, n, maxHsps, minScore), n, maxHsps);
}

HitAligner::HspLists HitAligner::align(const char* query, int32_t qlen, const ScanResult& r, int maxHsps, int minScore) {
    return align(query, qlen, r.referenceIds.data(), r.scores.data(), r.scores.size(), maxHsps, minScore);
}

HitAligner::HspLists HitAligner::align(const int8_t* pssm, int32_t qlen, const char* consensus, const int64_t* ids,
                                       const int32_t* scores, size_t n, int maxHsps, int minScore) {
    return trimmed(alignSlots(pssm, qlen, consensus, ids, scores, n, maxHsps, minScore), n, maxHsps);
}

HitAligner::HspLists HitAligner::align(const int8_t* pssm, int32_t qlen, const char* consensus, const ScanResult& r, int maxHsps,
                                       int minScore) {
    return align(pssm, qlen, consensus, r.referenceIds.data(), r.scores.data(), r.scores.size(), maxHsps, minScore);
}

std::vector<HitAlignment> HitAligner::align(const int8_t* pssm, int32_t qlen, const char* consensus, const ScanResult& r) {
    return align(pssm, qlen, consensus, r.referenceIds.data(), r.scores.data(), r.scores.size());
}

std::vector<HitAlignment> HitAligner::align(const int8_t* pssm, int32_t qlen, const char* consensus, const int64_t* ids,
                                            const int32_t* scores, size_t n) {
    residentHits_ = 0;
    if (n == 0) return std::vector<HitAlignment>();
    if (qlen <= 0 || !pssm || !ids || !scores) throw std::runtime_error("hit alignment: empty PSSM or null hit list");
    const std::vector<int8_t> c = encodeConsensus(pssm, qlen, consensus);
    return run(consensus ? c.data() : nullptr, pssm, qlen, ids, scores, n);
}

std::vector<HitAlignment> HitAligner::run(const int8_t* codes, const int8_t* pssm, int32_t qlen, const int64_t* ids,
                                          const int32_t* scores, size_t n, int maxHsps, int minScore) {
    const size_t H = size_t(maxHsps), slots = n * H;   // records and CIGAR slots: slot (i, k) at i * H + k
    std::vector<HitAlignment> out(slots);
    // the hit subjects in dbdata layout, from the host copy of the DB (resident, streamed, pseudo and array DBs alike)
    std::vector<int8_t> chars;
    std::vector<uint64_t> offsets(n + 1, 0);
    std::vector<int32_t> lengths(n);
    std::vector<int64_t> cigarOffsets(slots + 1, 0);
    int32_t maxLen = 0;
    size_t traceBytes = 0;
    for (size_t i = 0; i < n; i++) {
        const std::string s = d_.getReferenceSequence(ids[i]);
        lengths[i] = int32_t(s.size());
        maxLen = std::max(maxLen, lengths[i]);
        const size_t padded = (s.size() + 3) / 4 * 4;
        chars.resize(size_t(offsets[i]) + padded, kOtherCode);
        for (size_t k = 0; k < s.size(); k++) chars[size_t(offsets[i]) + k] = encode_residue(s[k]);
        // what the scan scored is the masked subject: the score check below holds the two statements together
        if (d_.masksSubjects()) mask_subject(chars.data() + offsets[i], lengths[i], d_.maskParams(), chars.data() + offsets[i]);
        offsets[i + 1] = offsets[i] + padded;
        for (size_t k = 0; k < H; k++) cigarOffsets[i * H + k + 1] = cigarOffsets[i * H + k] + qlen + lengths[i];
        traceBytes = std::max(traceBytes, trace_bytes_for(size_t(qlen), s.size()));
    }
    // trace budget: every pair's whole matrix if one pair's share fits --maxTempBytes; otherwise what fits, and the
    // pairs over it report coordinates only (SW_ALIGN_NO_TRACE)
    const size_t maxTemp = d_.memoryConfig().maxTempBytes;
    const size_t border = round_up(sizeof(int32_t) * 2 * (size_t(maxLen) + 1));
    // (the used pairs of the alignments before the last, sw_align_hsps' share of a pair's scratch, come first)
    const size_t fixed = border + round_up(sizeof(int32_t) * (H - 1) * size_t(qlen));
    if (fixed + round_up(traceBytes) > maxTemp) traceBytes = maxTemp > fixed + 256 ? (maxTemp - fixed) / 256 * 256 : 0;
    const size_t slot = fixed + round_up(traceBytes);
    const size_t tempBytes = std::min(slot * n, std::max(maxTemp / slot, size_t(1)) * slot);

    hip_check(hipSetDevice(device_), "hipSetDevice");
    auto put = [&](int b, const void* src, size_t bytes) {
        void* dst = grow(size_t(b), bytes);
        hip_check(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream_), "hipMemcpyAsync");
        return dst;
    };
    sw_align_args a{};
    a.query = codes ? static_cast<const int8_t*>(put(kQuery, codes, size_t(qlen))) : nullptr;
    const int8_t* devPssm = pssm ? static_cast<const int8_t*>(put(kPssm, pssm, size_t(qlen) * SW_PSSM_COLUMNS)) : nullptr;
    a.qlen = qlen;
    a.n = int32_t(n);
    a.chars = static_cast<const int8_t*>(put(kChars, chars.data(), chars.size()));
    a.offsets = static_cast<const uint64_t*>(put(kOffsets, offsets.data(), offsets.size() * sizeof(uint64_t)));
    a.lengths = static_cast<const int32_t*>(put(kLengths, lengths.data(), lengths.size() * sizeof(int32_t)));
    a.max_subject_len = maxLen;
    a.gop = d_.gapOpen();
    a.gex = d_.gapExtend();
    a.expected_scores = static_cast<const int32_t*>(put(kScores, scores, n * sizeof(int32_t)));
    a.results = static_cast<sw_align_result*>(grow(kResults, slots * sizeof(sw_align_result)));
    a.cigar = static_cast<uint32_t*>(grow(kCigar, size_t(cigarOffsets[slots]) * sizeof(uint32_t)));
    a.cigar_offsets = static_cast<const int64_t*>(put(kCigarOffsets, cigarOffsets.data(), cigarOffsets.size() * sizeof(int64_t)));
    a.trace_bytes = traceBytes;
    a.temp = grow(kTemp, tempBytes);
    a.temp_bytes = tempBytes;
    a.stream = stream_;
    if (maxHsps > 1) {
        const sw_hsp_args h{maxHsps, minScore};
        if (pssm) sw_check(sw_align_hsps_pssm(ctx_, &a, &h, devPssm), "sw_align_hsps_pssm");
        else sw_check(sw_align_hsps(ctx_, &a, &h), "sw_align_hsps");
        // resident(): the first alignments as n records of their own (their cigar_offset still points into the CIGAR buffer)
        void* first = grow(kFirstResults, n * sizeof(sw_align_result));
        hip_check(hipMemcpy2DAsync(first, sizeof(sw_align_result), a.results, H * sizeof(sw_align_result), sizeof(sw_align_result), n,
                                   hipMemcpyDeviceToDevice, stream_), "hipMemcpy2DAsync");
    } else if (pssm) {
        sw_check(sw_align_hits_pssm(ctx_, &a, devPssm), "sw_align_hits_pssm");
    } else {
        sw_check(sw_align_hits(ctx_, &a), "sw_align_hits");
    }
    residentFirst_ = maxHsps > 1;
    std::vector<sw_align_result> res(slots);
    std::vector<uint32_t> cigar(static_cast<size_t>(cigarOffsets[slots]));
    hip_check(hipMemcpyAsync(res.data(), a.results, slots * sizeof(sw_align_result), hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync");
    hip_check(hipMemcpyAsync(cigar.data(), a.cigar, cigar.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync");
    hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    for (size_t i = 0; i < slots; i++) {
        if (res[i].status == SW_ALIGN_SCORE_MISMATCH)
            throw std::runtime_error("hit alignment: subject " + std::to_string(ids[i / H]) + " scores " + std::to_string(res[i].score) +
                                     ", the scan reported " + std::to_string(scores[i / H]));
        if (res[i].status == SW_ALIGN_BAD_LENGTH) throw std::runtime_error("hit alignment: internal error (subject length bound)");
        out[i].r = res[i];
        out[i].r.cigar_offset = 0;
        const uint32_t* w = cigar.data() + res[i].cigar_offset;
        out[i].cigar.assign(w, w + res[i].cigar_len);
    }
    residentHits_ = n;
    return out;
}

HitAligner::Resident HitAligner::resident() const {
    Resident r;
    r.device = device_;
    r.ctx = ctx_;
    r.stream = stream_;
    r.n = residentHits_;
    if (r.n) {
        r.chars = static_cast<const int8_t*>(buf_[kChars]);
        r.offsets = static_cast<const uint64_t*>(buf_[kOffsets]);
        r.lengths = static_cast<const int32_t*>(buf_[kLengths]);
        r.results = static_cast<const sw_align_result*>(buf_[residentFirst_ ? kFirstResults : kResults]);
        r.cigar = static_cast<const uint32_t*>(buf_[kCigar]);
    }
    return r;
}

}  // namespace swh

#ifdef SWH_DRIVER_CAPI   // libcudasw4_host.so (with driver_capi.cpp); `align` links the class alone
namespace {

// query != nullptr: the letter form; else the PSSM form
// max_hsps == 0: the plain calls (n records); else n * max_hsps records, slot (i, k) at i * max_hsps + k
int align_hits_capi(swdrv* d, const char* query, const int8_t* pssm, const char* consensus, int32_t qlen, const int64_t* ids,
                    const int32_t* scores, int n, sw_align_result* results, uint32_t* cigar, int64_t cigar_cap, int max_hsps = 0,
                    int min_score = 1) {
    try {
        if (!d || !d->driver) throw std::runtime_error("null driver");
        if (n < 0 || (n > 0 && (!results || (!cigar && cigar_cap > 0)))) throw std::runtime_error("bad output arguments");
        swh::HitAligner aligner(*d->driver);
        const std::vector<swh::HitAlignment> hits =
            max_hsps ? (pssm ? aligner.alignSlots(pssm, qlen, consensus, ids, scores, size_t(n), max_hsps, min_score)
                             : aligner.alignSlots(query, qlen, ids, scores, size_t(n), max_hsps, min_score))
                     : (pssm ? aligner.align(pssm, qlen, consensus, ids, scores, size_t(n))
                             : aligner.align(query, qlen, ids, scores, size_t(n)));
        int64_t used = 0;
        for (size_t i = 0; i < hits.size(); i++) {
            results[i] = hits[i].r;
            results[i].cigar_offset = used;
            if (used + int64_t(hits[i].cigar.size()) > cigar_cap) throw std::runtime_error("cigar_cap too small");
            std::copy(hits[i].cigar.begin(), hits[i].cigar.end(), cigar + used);
            used += int64_t(hits[i].cigar.size());
        }
        return 0;
    } catch (const std::exception& e) {
        swh::set_driver_error(e.what());
        return -1;
    }
}

}  // namespace

extern "C" int swdrv_align_hits(swdrv* d, const char* query, int32_t qlen, const int64_t* ids, const int32_t* scores, int n,
                                sw_align_result* results, uint32_t* cigar, int64_t cigar_cap) {
    return align_hits_capi(d, query, nullptr, nullptr, qlen, ids, scores, n, results, cigar, cigar_cap);
}

extern "C" int swdrv_align_hits_pssm(swdrv* d, const int8_t* pssm, int32_t qlen, const char* consensus, const int64_t* ids,
                                     const int32_t* scores, int n, sw_align_result* results, uint32_t* cigar, int64_t cigar_cap) {
    if (!pssm) {
        swh::set_driver_error("hit alignment: null PSSM");
        return -1;
    }
    return align_hits_capi(d, nullptr, pssm, consensus, qlen, ids, scores, n, results, cigar, cigar_cap);
}

extern "C" int swdrv_align_hsps(swdrv* d, const char* query, int32_t qlen, const int64_t* ids, const int32_t* scores, int n,
                                int max_hsps, int min_score, sw_align_result* results, uint32_t* cigar, int64_t cigar_cap) {
    if (max_hsps < 1) {
        swh::set_driver_error("hit alignment: max_hsps must lie in [1, " + std::to_string(SW_MAX_HSPS) + "]");
        return -1;
    }
    return align_hits_capi(d, query, nullptr, nullptr, qlen, ids, scores, n, results, cigar, cigar_cap, max_hsps, min_score);
}

extern "C" int swdrv_align_hsps_pssm(swdrv* d, const int8_t* pssm, int32_t qlen, const char* consensus, const int64_t* ids,
                                     const int32_t* scores, int n, int max_hsps, int min_score, sw_align_result* results,
                                     uint32_t* cigar, int64_t cigar_cap) {
    if (!pssm || max_hsps < 1) {
        swh::set_driver_error(!pssm ? "hit alignment: null PSSM" : "hit alignment: max_hsps must lie in [1, " + std::to_string(SW_MAX_HSPS) + "]");
        return -1;
    }
    return align_hits_capi(d, nullptr, pssm, consensus, qlen, ids, scores, n, results, cigar, cigar_cap, max_hsps, min_score);
}
#endif
