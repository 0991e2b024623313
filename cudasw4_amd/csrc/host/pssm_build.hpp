// pssm_build.hpp — building a PSSM from a query's aligned hits (DESIGN.md "Building a PSSM"): the conversion of the device's
// weighted residue counts (sw_pssm_accumulate, include/cudasw4_amd_pssm.h) into the qlen x 21 int8 PSSM every scan takes,
// and the step around it: align the hits, apply the inclusion rule, accumulate on the device, convert.  An extension.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "hit_alignment.hpp"
#include "hit_msa.hpp"
#include "search_driver.hpp"
#include "sequence_codec.hpp"

namespace swh {

// the 21-letter table a matrix stands for when a PSSM is built (a 25-letter matrix: the 21-letter table of the same name)
const SubstitutionMatrix& pssm_table_of(MatrixId id);

// the positive root of sum_ab p_a p_b exp(lambda s_ab) = 1 over the 20 standard residues of a 21 x 21 table, p = the
// Robinson & Robinson background frequencies; bisection on [1e-3, 2] to the last bit
double pssm_lambda(const SubstitutionMatrix& table21);

// The conversion (pure host code).  master: qlen dbdata codes; counts / wcounts: qlen x 20; pseudocount > 0; out: qlen x 21;
// raw (optional): qlen x 20 scores before rounding; lambda (optional).  Throws std::runtime_error on a pseudocount that is
// not positive and on a table whose column 20 is not negative.
void pssm_from_counts(const SubstitutionMatrix& table21, const int8_t* master, int32_t qlen, const uint32_t* counts,
                      const uint64_t* wcounts, double pseudocount, int8_t* out, double* raw, double* lambda);

struct PssmBuildInfo {
    int32_t used = 0;         // hits that took part
    int32_t belowScore = 0;   // left out: scan score below the inclusion score
    int32_t noTrace = 0;      // left out: SW_ALIGN_NO_TRACE
    int32_t copies = 0;       // left out: a copy of the master
    int32_t purged = 0;       // left out: redundant to the master or to an earlier hit that went in (purgeIdentity > 0)
    double lambda = 0;
    std::vector<uint8_t> included;   // one byte per hit: 1 where it took part
    std::vector<HitAlignment> alignments;   // the hits as they were aligned for this step
    // built with maxHsps > 1: all alignments of every hit (HitAligner::HspLists; element 0 = `alignments`); else empty
    HitAligner::HspLists hsps;
};

// One step of an iterated search on the aligner's device, stream and buffers: the hits' subjects, results and CIGARs stay
// where HitAligner::align left them and are accumulated there.
class PssmBuilder {
public:
    PssmBuilder(const SearchDriver& driver, HitAligner& aligner) : d_(driver), aligner_(aligner) {}
    ~PssmBuilder();
    PssmBuilder(const PssmBuilder&) = delete;
    PssmBuilder& operator=(const PssmBuilder&) = delete;

    // master: the original query's letters (for a PSSM input the residue column of its file).  pssm: nullptr when the hits
    // were scanned with the letters, else the qlen x 21 PSSM they were scanned with.  admitted: nullptr, or one byte per hit
    // that takes the place of the score test (inclusion by E-value: 0 = left out, counted in belowScore).  -> qlen x 21 int8
    // maxHsps > 1: the hits are aligned with up to maxHsps alignments each, the further ones scoring at least hspMinScore
    // (info->hsps); the PSSM is built from the first alignments (HitAligner::resident()) and is the one of maxHsps == 1.
    // purgeIdentity P in 1 .. 100 (0: none): the hits that pass the rules above go through the redundancy filter of
    // sw_msa_filter (hit_msa.hpp), in rank order behind the master, and the purged ones are left out before the weighting.
    std::vector<int8_t> build(const char* master, int32_t qlen, const int8_t* pssm, const int64_t* ids, const int32_t* scores,
                              size_t n, int32_t minScore, double pseudocount, PssmBuildInfo* info, const uint8_t* admitted = nullptr,
                              int maxHsps = 1, int hspMinScore = 1, int purgeIdentity = 0);

private:
    void* grow(int slot, size_t bytes);
    const SearchDriver& d_;
    HitAligner& aligner_;
    std::unique_ptr<HitMsa> msa_;   // made by the first build with purgeIdentity > 0
    int device_ = -1;
    enum { kMaster, kInclude, kCounts, kWeights, kWcounts, kUsed, kBuffers };
    void* buf_[kBuffers] = {};
    size_t cap_[kBuffers] = {};
};

}  // namespace swh
