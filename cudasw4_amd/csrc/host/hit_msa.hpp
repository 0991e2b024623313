// hit_msa.hpp — the query-anchored multiple alignment of a query's aligned hits: the redundancy filter on the
// device (sw_msa_filter, include/cudasw4_amd_msa.h), run on what HitAligner::align left there, and the A3M / FASTA writer.
// An extension.
#pragma once
#include <cstddef>
#include <cstdint>
#include <iosfwd>
#include <string>
#include <vector>

#include "hit_alignment.hpp"

namespace swh {

struct MsaFilterResult {
    std::vector<uint8_t> keep;        // n + 1, entry n the master's
    std::vector<int32_t> residues;    // n + 1
    int32_t purged = 0;
    std::vector<uint8_t> rows;        // (n + 1) x qlen when asked for, else empty
};

// The selection of DESIGN.md §18 (sw_msa_select, include/cudasw4_amd_msa_select.h): 0 switches a test off.
struct MsaSelectParams {
    int minCoverage = 0;              // C: per cent of the query's positions a hit must have aligned
    int minQueryIdentity = 0;         // Q: per cent of a hit's residues that must equal the master's
    int diff = 0;                     // D: a hit is kept only while some column of it has fewer than D kept residues
    std::vector<int32_t> ladder{90};  // strictly ascending identity thresholds, 1 .. 16 values in 1 .. 100
};

struct MsaSelectResult {
    std::vector<uint8_t> state;       // n + 1 (SW_MSA_STATE_*), entry n the master's
    std::vector<int32_t> residues;    // n + 1
    int32_t counts[4] = {0, 0, 0, 0};  // kept hits, below coverage, below query identity, thinned
    std::vector<int32_t> depth;       // qlen
    std::vector<uint8_t> rows;        // (n + 1) x qlen when asked for, else empty
};

// Runs sw_msa_filter / sw_msa_select on HitAligner::resident(): the aligner's device, context and stream, buffers of its own that grow on
// demand.  Valid between an align() and the next one.
class HitMsa {
public:
    explicit HitMsa(HitAligner& aligner) : aligner_(aligner) {}
    ~HitMsa();
    HitMsa(const HitMsa&) = delete;
    HitMsa& operator=(const HitMsa&) = delete;

    // master: qlen residue letters (encode_residue; nullptr: no master row).  include: nullptr or one byte per resident hit.
    // maxIdentity: 0 (no filter) or 1 .. 100.
    MsaFilterResult filter(const char* master, int32_t qlen, const uint8_t* include, int maxIdentity, bool wantRows);
    // the same inputs through sw_msa_select; at most SW_MSA_SELECT_MAX_HITS resident hits
    MsaSelectResult select(const char* master, int32_t qlen, const uint8_t* include, const MsaSelectParams& params, bool wantRows);

private:
    void* grow(int slot, size_t bytes);
    HitAligner& aligner_;
    int device_ = -1;
    enum { kMaster, kInclude, kRows, kResidues, kKeep, kPurged, kTemp, kState, kCounts, kDepth, kBuffers };
    void* buf_[kBuffers] = {};
    size_t cap_[kBuffers] = {};
};

enum class MsaFormat { A3m, Fasta };
bool parse_msa_format(const std::string& name, MsaFormat& out);   // "a3m" | "fasta"

// One sequence line: '-' before q_begin, along the CIGAR the subject's letters in upper case for '=' / 'X', '-' per 'I'
// column, the subject's letters in lower case for 'D' (Fasta: none), then '-' up to qlen.  Positions outside the subject
// print 'X' / 'x'.  Upper-case letters plus '-' number exactly qlen.
std::string msa_line(MsaFormat format, int32_t qlen, const std::string& subjectLetters, const HitAlignment& a);

// The writer (pure host): '>' + queryHeader and the master's letters, then for every hit with keep[h] != 0 (keep == nullptr:
// every hit) that is SW_ALIGN_OK with a CIGAR, in rank order, '>' + its header unchanged and its line.  -> hits written
size_t write_msa(std::ostream& os, MsaFormat format, const std::string& master, const std::string& queryHeader,
                 const std::vector<std::string>& headers, const std::vector<std::string>& subjectLetters,
                 const std::vector<HitAlignment>& alignments, const uint8_t* keep);
size_t write_msa(const std::string& path, MsaFormat format, const std::string& master, const std::string& queryHeader,
                 const std::vector<std::string>& headers, const std::vector<std::string>& subjectLetters,
                 const std::vector<HitAlignment>& alignments, const uint8_t* keep);

}  // namespace swh
