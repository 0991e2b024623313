// cli_options.hpp — command line of `align`, flag-for-flag the reference's (options.hpp:9-51,
// options.cpp:47-267).
#pragma once
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "search_driver.hpp"
#include "sequence_codec.hpp"

namespace swh {

struct ProgramOptions {
    enum class OutputMode { Plain, TSV };
    bool help = false;
    bool loadFullDBToGpu = false;
    bool usePseudoDB = false;
    bool printLengthPartitions = false;
    bool interactive = false;
    bool verbose = false;
    bool alignments = false;     // --alignments: coordinates and CIGAR of every result (hit_alignment.hpp); an extension
    // --pssmAlignments: --alignments for every query of the command line, --pssm queries included (identities and '=' / 'X'
    // of a PSSM against the residue column of its file)
    bool pssmAlignments = false;
    bool reportAlignments() const { return alignments || pssmAlignments; }
    // --maxHsps N --hspMinScore S (with --alignments / --pssmAlignments; hit_alignment.hpp): up to N
    // non-overlapping alignments per result, the further ones scoring at least S; checked in main, before any device is opened
    bool haveMaxHsps = false;
    int maxHsps = 1;
    bool haveHspMinScore = false;
    int hspMinScore = 1;
    bool reportHsps() const { return maxHsps > 1; }
    // Iterated profile search (pssm_build.hpp; an extension): --iterations N rounds, each scanning with the PSSM built from
    // the round before's reported hits of raw score >= --inclusionScore (or by E-value: --inclusionEvalue below); --pseudocount is the
    // conversion's beta; --outPssm PREFIX writes PREFIX.<query number>.pssm
    int iterations = 1;
    bool haveInclusionScore = false;
    int inclusionScore = 0;
    double pseudocount = 10.0;
    std::string outPssm;
    bool buildsPssm() const { return iterations > 1 || !outPssm.empty(); }
    // Search statistics (search_stats.hpp; an extension): --evalues reports a Z-score and an E-value with every result;
    // --maxEvalue X (implies --evalues) prints only the results with E <= X; --inclusionEvalue X takes the place of
    // --inclusionScore: results go into the PSSM by their E-value under the round's own fit
    bool evalues = false;
    bool haveMaxEvalue = false;
    double maxEvalue = 0;
    bool haveInclusionEvalue = false;
    double inclusionEvalue = 0;
    // --rankBy score|evalue (search_rank.hpp; an extension): evalue ranks the --top list by E-value instead of raw score,
    // implies --evalues and scans one query at a time; the value is checked in main, before any device is opened
    bool haveRankBy = false;
    std::string rankBy = "score";
    bool rankByEvalue() const { return rankBy == "evalue"; }
    // --statistics scan|shuffled (shuffle_stats.hpp; an extension): shuffled fits every query's statistics on its scores against
    // a sample of the DB with permuted subjects (--shuffleSubjects M of them, --shuffles R times each, --shuffleSeed S), implies
    // --evalues and scans one query at a time; the values are checked in main, before any device is opened
    bool haveStatistics = false;
    std::string statistics = "scan";
    bool haveShuffles = false, haveShuffleSubjects = false, haveShuffleSeed = false;
    long long shuffles = 0;            // 0: ceil(2000 / sample) clamped to 1 .. 64
    long long shuffleSubjects = 10000;
    unsigned long long shuffleSeed = 1;
    bool shuffledStatistics() const { return statistics == "shuffled"; }
    bool reportEvalues() const { return evalues || haveMaxEvalue || rankByEvalue() || shuffledStatistics(); }
    bool wantStatistics() const { return reportEvalues() || haveInclusionEvalue; }
    // --maskSubjects (subject_mask.hpp; an extension): low-complexity segments of the subjects are masked on the
    // GPU before anything scans them; --maskWindow W, --maskTrigger K1 and --maskExtend K2 (entropies in bits) replace the
    // defaults.  The values are kept as given and checked in main, before any device is opened.
    bool maskSubjects = false;
    bool haveMaskWindow = false, haveMaskTrigger = false, haveMaskExtend = false;
    std::string maskWindow = "12", maskTrigger = "1.9", maskExtend = "2.2";
    // The query-anchored MSA of a query's results (hit_msa.hpp; an extension): --outMsa PREFIX writes
    // PREFIX.<query number>.a3m (--msaFormat fasta: .fasta) from the reported results of the query's last round; --msaMaxIdentity P
    // leaves out results that are at least P per cent identical to the query or to a result written before them;
    // --purgeIdentity P does the same to the results that go into a PSSM.  The values are kept as given and checked in main,
    // before any device is opened (which fills the two numbers; 0: no filter).
    std::string outMsa;
    bool haveOutMsa = false, haveMsaFormat = false, haveMsaMaxIdentity = false, havePurgeIdentity = false;
    std::string msaFormat = "a3m", msaMaxIdentityText, purgeIdentityText;
    int msaMaxIdentity = 0, purgeIdentity = 0;
    bool writesMsa() const { return haveOutMsa; }
    // The selection of the rows that are written (an extension): --msaMinCoverage C, --msaMinQueryIdentity Q,
    // --msaDiff D and --msaDiffLadder p0,p1,...  Kept as given and checked in main, before any device is opened, which
    // fills the numbers and the ladder.  With any of them the file is written from sw_msa_select's states.
    bool haveMsaMinCoverage = false, haveMsaMinQueryIdentity = false, haveMsaDiff = false, haveMsaDiffLadder = false;
    std::string msaMinCoverageText, msaMinQueryIdentityText, msaDiffText, msaDiffLadderText;
    int msaMinCoverage = 0, msaMinQueryIdentity = 0, msaDiff = 0;
    std::vector<int32_t> msaLadder;
    bool selectsMsaRows() const { return haveMsaMinCoverage || haveMsaMinQueryIdentity || haveMsaDiff || haveMsaDiffLadder; }
    bool prefetchDBFile = false;
    int numTopOutputs = 10;
    int gop = -11;
    int gex = -1;
    // --refCompat (or CUDASW4_AMD_REF_COMPAT=1): score exactly like the reference BINARY.  There --gop / --gex and the
    // per-matrix default gap scores are parsed and printed (options.cpp:179-194) but never reach the kernels
    // (cudasw4.cuh:539-550: the setters have no call site), which always run gop -11 / gex -1 — so the same inputs give the
    // reference's output for every --mat.  The reference's other quirk, the fp16 overflow check that is off for partitions
    // 0-12, is NOT reproduced: it returns inexact scores.
    bool refCompat = false;
    int effectiveGop() const { return refCompat ? -11 : gop; }
    int effectiveGex() const { return refCompat ? -1 : gex; }
    int pseudoDBLength = 0;
    int pseudoDBSize = 0;
    MatrixId matrix = MatrixId::Blosum62;
    KernelTypeConfig kernels;
    OutputMode outputMode = OutputMode::Plain;
    MemoryConfig memory;
    std::string outputfile = "/dev/stdout";
    std::string dbPrefix;
    std::vector<std::string> queryFiles;
    // --pssm: NCBI ASCII PSSM files, each one query (pssm_query.hpp); `inputs` keeps --query and --pssm in the order given
    std::vector<std::string> pssmFiles;
    struct QueryInput { std::string path; bool pssm; };
    std::vector<QueryInput> inputs;
};

void printOptions(const ProgramOptions& options);
bool parseArgs(int argc, char** argv, ProgramOptions& options);
void printHelp(char** argv);
size_t parseMemoryString(const std::string& s);

}  // namespace swh
