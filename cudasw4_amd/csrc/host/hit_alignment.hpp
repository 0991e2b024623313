// hit_alignment.hpp — coordinates and CIGAR of a scan's top hits (sw_align_hits, include/cudasw4_amd.h; for the hits of a
// PSSM query sw_align_hits_pssm, include/cudasw4_amd_pssm.h), run after SearchDriver::collect(); with maxHsps > 1 up to that
// many non-overlapping alignments per hit (sw_align_hsps, include/cudasw4_amd_hsps.h).  An extension: the reference
// reports scores only.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../../include/cudasw4_amd.h"
#include "search_driver.hpp"

namespace swh {

struct HitAlignment {
    sw_align_result r;            // cigar_offset: 0 (the words are in `cigar`)
    std::vector<uint32_t> cigar;  // len << 4 | op words
};

std::string cigar_string(const std::vector<uint32_t>& words);   // "*" when empty

// Aligns hits on the device of the driver's first GPU with a context and a stream of its own (a context is driven by one
// host thread, and the driver's workers may already scan the next query).  Device buffers grow on demand.
class HitAligner {
public:
    explicit HitAligner(const SearchDriver& driver);
    ~HitAligner();
    HitAligner(const HitAligner&) = delete;
    HitAligner& operator=(const HitAligner&) = delete;

    // query: residue letters of the query the hits were scanned with; ids / scores: the hits (global ids, scan scores).
    // A hit whose recomputed score differs from its scan score is an error.
    std::vector<HitAlignment> align(const char* query, int32_t qlen, const int64_t* ids, const int32_t* scores, size_t n);
    std::vector<HitAlignment> align(const char* query, int32_t qlen, const ScanResult& r);

    // The hits of a PSSM query (pssm: qlen x 21 int8 row-major, host; column 20 negative in every row).  consensus: qlen
    // residue letters that '=' / 'X' and the identities are counted against (encode_residue: a non-standard letter, '*'
    // or '-' is identical to nothing), or nullptr: the best-scoring standard residue of every row.  The driver's gap
    // scores apply, its matrix does not.
    std::vector<HitAlignment> align(const int8_t* pssm, int32_t qlen, const char* consensus, const int64_t* ids,
                                    const int32_t* scores, size_t n);
    std::vector<HitAlignment> align(const int8_t* pssm, int32_t qlen, const char* consensus, const ScanResult& r);

    // Up to maxHsps (1 .. SW_MAX_HSPS) non-overlapping alignments per hit (sw_align_hsps / sw_align_hsps_pssm): one vector per
    // hit, element 0 = the alignment the calls above return (whatever its status), then the further alignments that are
    // SW_ALIGN_OK, best first; those scoring below minScore (>= 1) are not reported.  The trace budget is handled as above
    // (the used pairs of a hit take (maxHsps - 1) x qlen x 4 bytes of its share of --maxTempBytes).
    typedef std::vector<std::vector<HitAlignment>> HspLists;
    HspLists align(const char* query, int32_t qlen, const int64_t* ids, const int32_t* scores, size_t n, int maxHsps, int minScore);
    HspLists align(const char* query, int32_t qlen, const ScanResult& r, int maxHsps, int minScore);
    HspLists align(const int8_t* pssm, int32_t qlen, const char* consensus, const int64_t* ids, const int32_t* scores, size_t n,
                   int maxHsps, int minScore);
    HspLists align(const int8_t* pssm, int32_t qlen, const char* consensus, const ScanResult& r, int maxHsps, int minScore);
    // the same untrimmed: n x maxHsps records, slot (i, k) at i * maxHsps + k, as sw_align_hsps wrote them
    std::vector<HitAlignment> alignSlots(const char* query, int32_t qlen, const int64_t* ids, const int32_t* scores, size_t n,
                                         int maxHsps, int minScore);
    std::vector<HitAlignment> alignSlots(const int8_t* pssm, int32_t qlen, const char* consensus, const int64_t* ids,
                                         const int32_t* scores, size_t n, int maxHsps, int minScore);

    // What the last align() left on the device: the hits' subjects, results and CIGAR words in the layout sw_align_hits
    // was given them, for a consumer that goes on with them there (pssm_build.hpp).  All work of the aligner is complete
    // when align() returns; the pointers are valid until the next align().  n == 0: there was no such call, or no hit.
    // After a call with maxHsps > 1 these are the hits' FIRST alignments (slot 0 of every hit, gathered into n records).
    struct Resident {
        int device = 0;
        sw_ctx* ctx = nullptr;
        hipStream_t stream = nullptr;
        const int8_t* chars = nullptr;
        const uint64_t* offsets = nullptr;
        const int32_t* lengths = nullptr;
        const sw_align_result* results = nullptr;
        const uint32_t* cigar = nullptr;
        size_t n = 0;
    };
    Resident resident() const;

private:
    // both forms behind the encoding of the query.  pssm == nullptr: `codes` are the query's codes; else `codes` are the
    // consensus codes (nullptr: none).  -> n x maxHsps slots
    std::vector<HitAlignment> run(const int8_t* codes, const int8_t* pssm, int32_t qlen, const int64_t* ids,
                                  const int32_t* scores, size_t n, int maxHsps = 1, int minScore = 1);
    std::vector<int8_t> encodeQuery(const char* query, int32_t qlen) const;
    std::vector<int8_t> encodeConsensus(const int8_t* pssm, int32_t qlen, const char* consensus) const;
    void* grow(size_t slot, size_t bytes);
    const SearchDriver& d_;
    int device_ = 0;
    sw_ctx* ctx_ = nullptr;
    hipStream_t stream_ = nullptr;
    enum { kQuery, kPssm, kChars, kOffsets, kLengths, kScores, kResults, kCigar, kCigarOffsets, kTemp, kFirstResults, kBuffers };
    void* buf_[kBuffers] = {};
    size_t cap_[kBuffers] = {};
    size_t residentHits_ = 0;
    bool residentFirst_ = false;   // the last call had maxHsps > 1: resident().results are the gathered first alignments
};

}  // namespace swh
