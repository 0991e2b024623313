#include "cli_options.hpp"

#include <cstdlib>
#include <iostream>

namespace swh {

size_t parseMemoryString(const std::string& s) {
    if (s.empty()) return 0;
    size_t factor = 1;
    std::string digits = s;
    switch (s.back()) {
        case 'K': factor = size_t(1) << 10; digits.pop_back(); break;
        case 'M': factor = size_t(1) << 20; digits.pop_back(); break;
        case 'G': factor = size_t(1) << 30; digits.pop_back(); break;
        default: break;
    }
    return factor * std::stoull(digits);
}

void printOptions(const ProgramOptions& o) {
    std::cout << "Selected options:\n";
    std::cout << "verbose: " << o.verbose << "\n";
    std::cout << "interactive: " << o.interactive << "\n";
    std::cout << "loadFullDBToGpu: " << o.loadFullDBToGpu << "\n";
    std::cout << "prefetchDBFile: " << o.prefetchDBFile << "\n";
    std::cout << "numTopOutputs: " << o.numTopOutputs << "\n";
    std::cout << "gop: " << o.gop << "\n";
    std::cout << "gex: " << o.gex << "\n";
    if (o.refCompat) std::cout << "refCompat: gap scores applied are " << o.effectiveGop() << " / " << o.effectiveGex() << " like the reference binary's\n";
    std::cout << "maxBatchBytes: " << o.memory.maxBatchBytes << "\n";
    std::cout << "maxBatchSequences: " << o.memory.maxBatchSequences << "\n";
    std::cout << "maxTempBytes: " << o.memory.maxTempBytes << "\n";
    for (size_t i = 0; i < o.queryFiles.size(); i++) std::cout << "queryFile " << i << " : " << o.queryFiles[i] << "\n";
    for (size_t i = 0; i < o.pssmFiles.size(); i++) std::cout << "pssmFile " << i << " : " << o.pssmFiles[i] << "\n";
    if (o.pssmAlignments) std::cout << "pssmAlignments: " << o.pssmAlignments << "\n";
    if (o.reportHsps()) std::cout << "maxHsps: " << o.maxHsps << "\nhspMinScore: " << o.hspMinScore << "\n";
    if (o.iterations != 1) std::cout << "iterations: " << o.iterations << "\n";
    if (o.haveInclusionScore) std::cout << "inclusionScore: " << o.inclusionScore << "\n";
    if (o.haveInclusionEvalue) std::cout << "inclusionEvalue: " << o.inclusionEvalue << "\n";
    if (o.pseudocount != 10.0) std::cout << "pseudocount: " << o.pseudocount << "\n";
    if (o.reportEvalues()) std::cout << "evalues: 1\n";
    if (o.haveMaxEvalue) std::cout << "maxEvalue: " << o.maxEvalue << "\n";
    if (o.haveRankBy) std::cout << "rankBy: " << o.rankBy << "\n";
    if (o.haveStatistics) std::cout << "statistics: " << o.statistics << "\n";
    if (o.haveShuffles) std::cout << "shuffles: " << o.shuffles << "\n";
    if (o.haveShuffleSubjects) std::cout << "shuffleSubjects: " << o.shuffleSubjects << "\n";
    if (o.haveShuffleSeed) std::cout << "shuffleSeed: " << o.shuffleSeed << "\n";
    if (o.maskSubjects) std::cout << "maskSubjects: 1\n";
    if (o.haveMaskWindow) std::cout << "maskWindow: " << o.maskWindow << "\n";
    if (o.haveMaskTrigger) std::cout << "maskTrigger: " << o.maskTrigger << "\n";
    if (o.haveMaskExtend) std::cout << "maskExtend: " << o.maskExtend << "\n";
    if (!o.outPssm.empty()) std::cout << "outPssm: " << o.outPssm << "\n";
    if (o.havePurgeIdentity) std::cout << "purgeIdentity: " << o.purgeIdentityText << "\n";
    if (o.haveOutMsa) std::cout << "outMsa: " << o.outMsa << "\n";
    if (o.haveMsaFormat) std::cout << "msaFormat: " << o.msaFormat << "\n";
    if (o.haveMsaMaxIdentity) std::cout << "msaMaxIdentity: " << o.msaMaxIdentityText << "\n";
    if (o.haveMsaMinCoverage) std::cout << "msaMinCoverage: " << o.msaMinCoverageText << "\n";
    if (o.haveMsaMinQueryIdentity) std::cout << "msaMinQueryIdentity: " << o.msaMinQueryIdentityText << "\n";
    if (o.haveMsaDiff) std::cout << "msaDiff: " << o.msaDiffText << "\n";
    if (o.haveMsaDiffLadder) std::cout << "msaDiffLadder: " << o.msaDiffLadderText << "\n";
    std::cout << "blosum: " << substitution_matrix(o.matrix).name << "\n";
    std::cout << "singlePassType: " << to_string(o.kernels.singlePassType) << "\n";
    std::cout << "manyPassType_small: " << to_string(o.kernels.manyPassType_small) << "\n";
    std::cout << "manyPassType_large: " << to_string(o.kernels.manyPassType_large) << "\n";
    std::cout << "overflowType: " << to_string(o.kernels.overflowType) << "\n";
    if (o.usePseudoDB) {
        std::cout << "Using built-in pseudo db with " << o.pseudoDBSize << " sequences of length " << o.pseudoDBLength << "\n";
    } else {
        std::cout << "Using db file: " << o.dbPrefix << "\n";
    }
    std::cout << "memory limit per gpu: "
              << (o.memory.maxGpuMem == std::numeric_limits<size_t>::max() ? std::string("unlimited") : std::to_string(o.memory.maxGpuMem))
              << "\n";
    std::cout << "Output mode: " << (o.outputMode == ProgramOptions::OutputMode::TSV ? "TSV" : "Plain") << "\n";
    std::cout << "Output file: " << o.outputfile << "\n";
}

bool parseArgs(int argc, char** argv, ProgramOptions& o) {
    bool gotQuery = false, gotDB = false, gotGex = false, gotGop = false, gotDPX = false;
    o.queryFiles.clear();
    o.pssmFiles.clear();
    o.inputs.clear();
    auto value = [&](int& i) -> std::string {
        if (i + 1 >= argc) { std::cout << "Missing value for " << argv[i] << "\n"; return std::string(); }
        return argv[++i];
    };
    auto kernelType = [&](int& i, KernelType& dst) {
        const std::string v = value(i);
        if (!parse_kernel_type(v, dst)) std::cout << "Unknown kernel type " << v << " (valid: Half2, DPXs16, DPXs32, Float)\n";
    };
    for (int i = 1; i < argc; i++) {
        const std::string arg = argv[i];
        if (arg == "--help") o.help = true;
        else if (arg == "--uploadFull") o.loadFullDBToGpu = true;
        else if (arg == "--verbose") o.verbose = true;
        else if (arg == "--interactive") o.interactive = true;
        else if (arg == "--alignments") o.alignments = true;
        else if (arg == "--pssmAlignments") o.pssmAlignments = true;
        else if (arg == "--maxHsps") { o.maxHsps = std::atoi(value(i).c_str()); o.haveMaxHsps = true; }
        else if (arg == "--hspMinScore") { o.hspMinScore = std::atoi(value(i).c_str()); o.haveHspMinScore = true; }
        else if (arg == "--iterations") o.iterations = std::atoi(value(i).c_str());
        else if (arg == "--inclusionScore") { o.inclusionScore = std::atoi(value(i).c_str()); o.haveInclusionScore = true; }
        else if (arg == "--inclusionEvalue") { o.inclusionEvalue = std::atof(value(i).c_str()); o.haveInclusionEvalue = true; }
        else if (arg == "--evalues") o.evalues = true;
        else if (arg == "--maxEvalue") { o.maxEvalue = std::atof(value(i).c_str()); o.haveMaxEvalue = true; }
        else if (arg == "--rankBy") { o.rankBy = value(i); o.haveRankBy = true; }
        else if (arg == "--statistics") { o.statistics = value(i); o.haveStatistics = true; }
        else if (arg == "--shuffles") { o.shuffles = std::atoll(value(i).c_str()); o.haveShuffles = true; }
        else if (arg == "--shuffleSubjects") { o.shuffleSubjects = std::atoll(value(i).c_str()); o.haveShuffleSubjects = true; }
        else if (arg == "--shuffleSeed") { o.shuffleSeed = std::strtoull(value(i).c_str(), nullptr, 10); o.haveShuffleSeed = true; }
        else if (arg == "--maskSubjects") o.maskSubjects = true;
        else if (arg == "--maskWindow") { o.maskWindow = value(i); o.haveMaskWindow = true; }
        else if (arg == "--maskTrigger") { o.maskTrigger = value(i); o.haveMaskTrigger = true; }
        else if (arg == "--maskExtend") { o.maskExtend = value(i); o.haveMaskExtend = true; }
        else if (arg == "--pseudocount") o.pseudocount = std::atof(value(i).c_str());
        else if (arg == "--outPssm") o.outPssm = value(i);
        else if (arg == "--purgeIdentity") { o.purgeIdentityText = value(i); o.havePurgeIdentity = true; }
        else if (arg == "--outMsa") { o.outMsa = value(i); o.haveOutMsa = true; }
        else if (arg == "--msaFormat") { o.msaFormat = value(i); o.haveMsaFormat = true; }
        else if (arg == "--msaMaxIdentity") { o.msaMaxIdentityText = value(i); o.haveMsaMaxIdentity = true; }
        else if (arg == "--msaMinCoverage") { o.msaMinCoverageText = value(i); o.haveMsaMinCoverage = true; }
        else if (arg == "--msaMinQueryIdentity") { o.msaMinQueryIdentityText = value(i); o.haveMsaMinQueryIdentity = true; }
        else if (arg == "--msaDiff") { o.msaDiffText = value(i); o.haveMsaDiff = true; }
        else if (arg == "--msaDiffLadder") { o.msaDiffLadderText = value(i); o.haveMsaDiffLadder = true; }
        else if (arg == "--printLengthPartitions") o.printLengthPartitions = true;
        else if (arg == "--prefetchDBFile") o.prefetchDBFile = true;
        else if (arg == "--top") o.numTopOutputs = std::atoi(value(i).c_str());
        else if (arg == "--gop") { o.gop = std::atoi(value(i).c_str()); gotGop = true; }
        else if (arg == "--gex") { o.gex = std::atoi(value(i).c_str()); gotGex = true; }
        else if (arg == "--maxBatchBytes") o.memory.maxBatchBytes = parseMemoryString(value(i));
        else if (arg == "--maxBatchSequences") o.memory.maxBatchSequences = size_t(std::atoll(value(i).c_str()));
        else if (arg == "--maxTempBytes") o.memory.maxTempBytes = parseMemoryString(value(i));
        else if (arg == "--maxGpuMem") o.memory.maxGpuMem = parseMemoryString(value(i));
        else if (arg == "--query") { o.queryFiles.push_back(value(i)); o.inputs.push_back({o.queryFiles.back(), false}); gotQuery = true; }
        else if (arg == "--pssm") { o.pssmFiles.push_back(value(i)); o.inputs.push_back({o.pssmFiles.back(), true}); gotQuery = true; }
        else if (arg == "--db") { o.dbPrefix = value(i); gotDB = true; }
        else if (arg == "--mat") {
            const std::string v = value(i);
            if (!parse_matrix_name(v, o.matrix)) std::cout << "Unknown matrix " << v << "\n";
        }
        else if (arg == "--singlePassType") kernelType(i, o.kernels.singlePassType);
        else if (arg == "--manyPassType_small") kernelType(i, o.kernels.manyPassType_small);
        else if (arg == "--manyPassType_large") kernelType(i, o.kernels.manyPassType_large);
        else if (arg == "--overflowType") kernelType(i, o.kernels.overflowType);
        else if (arg == "--pseudodb") {
            o.usePseudoDB = true;
            o.pseudoDBSize = std::atoi(value(i).c_str());
            o.pseudoDBLength = std::atoi(value(i).c_str());
            gotDB = true;
        }
        else if (arg == "--dpx") gotDPX = true;
        else if (arg == "--refCompat") o.refCompat = true;
        else if (arg == "--tsv") o.outputMode = ProgramOptions::OutputMode::TSV;
        else if (arg == "--of") o.outputfile = value(i);
        else std::cout << "Unexpected arg " << arg << "\n";
    }
    // matrix-specific default gap scores unless given (options.cpp:179-194).  Unlike the reference,
    // where these never reach the kernels, they are forwarded to the scan.
    const SubstitutionMatrix& m = substitution_matrix(o.matrix);
    if (!gotGop) o.gop = m.default_gop;
    if (!gotGex) o.gex = m.default_gex;
    if (const char* e = std::getenv("CUDASW4_AMD_REF_COMPAT")) o.refCompat = o.refCompat || e[0] == '1';
    if (gotDPX) {
        o.kernels.singlePassType = KernelType::DPXs16;
        o.kernels.manyPassType_small = KernelType::DPXs16;
        o.kernels.manyPassType_large = KernelType::DPXs32;
        o.kernels.overflowType = KernelType::DPXs32;
    }
    if (!gotQuery && !o.interactive && !o.help) { std::cout << "Query is missing\n"; return false; }
    if (!gotDB && !o.help) { std::cout << "DB prefix is missing\n"; return false; }
    return true;
}

void printHelp(char** argv) {
    ProgramOptions d;
    std::cout << "Usage: " << argv[0] << " [options]\n";
    std::cout << "The GPUs to use are set via HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES environment variables.\n";
    std::cout << "Options: \n";
    std::cout << "   Mandatory\n";
    std::cout << "      --query queryfile : Mandatory. Fasta or Fastq. Can be gzip'ed. Repeat this option for multiple query files\n";
    std::cout << "      --pssm pssmfile : A position-specific scoring matrix as a query, in place of or beside --query: an NCBI ASCII PSSM\n"
                 "        (psiblast -out_ascii_pssm). Repeat this option for multiple PSSMs. Alignments of its results: --pssmAlignments (not --alignments)\n";
    std::cout << "      --db dbPrefix : Mandatory. The DB to query against. The same dbPrefix as used for makedb\n\n";
    std::cout << "   Scoring\n";
    std::cout << "      --top val : Output the val best scores. Default val = " << d.numTopOutputs << "\n";
    std::cout << "      --gop val : Gap open score. Overwrites our blosum-dependent default score.\n";
    std::cout << "      --gex val : Gap extend score. Overwrites our blosum-dependent default score.\n";
    std::cout << "      --mat val: Set substitution matrix. Supported values: blosum45, blosum50, blosum62, blosum80. Default: blosum62\n"
                 "        (with suffix _25: the full 25-letter table for the query letters B, J, Z, X, *)\n\n";
    std::cout << "   Iterated profile search\n";
    std::cout << "      --iterations N : N rounds per query (N >= 1, default 1). Round r + 1 scans with the PSSM built from the results of round r\n"
                 "        (the --top list); the results printed are the last round's. Stops early when the set of included results repeats.\n";
    std::cout << "      --inclusionScore S : Results with a raw score of at least S go into the PSSM. --iterations above 1 and --outPssm need\n"
                 "        this option or --inclusionEvalue, not both.\n";
    std::cout << "      --inclusionEvalue X : Results with an E-value of at most X, under the statistics of the round's own scan, go into the PSSM.\n";
    std::cout << "      --pseudocount B : Weight of the substitution-matrix pseudo-frequencies, B > 0. Default val = " << d.pseudocount << "\n";
    std::cout << "      --outPssm PREFIX : Write the PSSM built from the last round's results to PREFIX.<query number>.pssm (NCBI ASCII, as --pssm reads)\n";
    std::cout << "      --purgeIdentity P : Before the results are weighted, leave out every one that is at least P per cent identical, over its own\n"
                 "        aligned residues, to the query or to a result that went in before it (P in 1 .. 100; PSI-BLAST purges at 94).\n"
                 "        Needs --iterations above 1 or --outPssm. Default: nothing is purged, the weights alone handle redundancy\n\n";
    std::cout << "   Multiple alignment\n";
    std::cout << "      --outMsa PREFIX : Write the query-anchored multiple alignment of every query's reported results (of the last round, against\n"
                 "        that round's scoring; first alignments only) to PREFIX.<query number>.a3m. Aligns the results itself without --alignments\n";
    std::cout << "      --msaFormat a3m|fasta : a3m (default): insertions relative to the query in lower case. fasta: insertions left out, every\n"
                 "        line as long as the query; the file is PREFIX.<query number>.fasta. Needs --outMsa\n";
    std::cout << "      --msaMaxIdentity P : Write only results that are less than P per cent identical to the query and to every result written\n"
                 "        before them (P in 1 .. 100, a greedy filter on the GPU). Needs --outMsa. Default: every aligned result is written\n";
    std::cout << "      --msaMinCoverage C : Write only results that align at least C per cent of the query's positions (C in 1 .. 100). Needs --outMsa\n";
    std::cout << "      --msaMinQueryIdentity Q : Write only results of whose aligned residues at least Q per cent equal the query's (Q in 1 .. 100).\n"
                 "        Needs --outMsa\n";
    std::cout << "      --msaDiff D : Write the most diverse results that leave at least D residues in every column where so many exist (D >= 1): the\n"
                 "        results are taken rung by rung of a rising identity ladder, each only while one of its columns has fewer than D\n"
                 "        residues and no written row is similar to it at the rung. Rungs: 20, 30, ... below --msaMaxIdentity (default 90),\n"
                 "        then that. At most --top 16384. Needs --outMsa\n";
    std::cout << "      --msaDiffLadder p0,p1,... : The rungs of --msaDiff: 1 .. 16 strictly ascending values in 1 .. 100; the last one is the identity cut,\n"
                 "        so --msaMaxIdentity cannot be given with it. Needs --msaDiff\n\n";
    std::cout << "   Search statistics\n";
    std::cout << "      --evalues : Report a Z-score and an E-value with every result: the scores of the whole scan are regressed on the\n"
                 "        logarithm of the subject length (as FASTA / SSEARCH do), fitted per query on the GPU's score histogram. Two more TSV\n"
                 "        columns behind all others; '*' where the scan allows no fit (fewer than 100 usable scores, or no spread).\n";
    std::cout << "      --maxEvalue X : Implies --evalues. Print only the results of the --top list with an E-value of at most X.\n";
    std::cout << "      --rankBy score|evalue : What the --top list is ranked by. Default: score. evalue implies --evalues: the list holds the\n"
                 "        results of smallest E-value (largest Z-score) of the whole DB, not the best raw scores, which favour long subjects;\n"
                 "        queries are scanned one at a time. With --maxEvalue X and --verbose, also the number of subjects of the DB with an\n"
                 "        E-value of at most X. The raw-score list where the scan allows no fit.\n";
    std::cout << "      --statistics scan|shuffled : What the Z-scores and E-values are fitted on. Default: scan, the scan's own scores, which\n"
                 "        assumes that almost every subject is unrelated to the query. shuffled implies --evalues: every query is also scored\n"
                 "        against a sample of the DB whose subjects' residues are permuted on the GPU (length and composition kept, homology\n"
                 "        destroyed) and the fit is made on those scores - for DBs dominated by one family, and for DBs too small to fit.\n"
                 "        Queries are scanned one at a time.\n";
    std::cout << "      --shuffleSubjects M : With --statistics shuffled: the sample holds at most M subjects, evenly spread over the DB's length\n"
                 "        order. Default: 10000.\n";
    std::cout << "      --shuffles R : With --statistics shuffled: every subject of the sample is permuted R times (1 .. 64). Default: as many as\n"
                 "        bring 2000 scores, 1 .. 64.\n";
    std::cout << "      --shuffleSeed S : With --statistics shuffled: seed of the permutations. Default: 1.\n\n";
    std::cout << "   Subject masking\n";
    std::cout << "      --maskSubjects : Mask low-complexity segments of the subjects (poly-Q, S/G/A-rich linkers, short repeats) on the GPU before\n"
                 "        they are scanned: the trigger and extension stages of SEG on a fixed window. A masked residue scores like X; alignments\n"
                 "        and PSSMs see the masked subject. With --verbose, one line per query with the residues and subjects masked.\n";
    std::cout << "      --maskWindow W : With --maskSubjects: the window, 4 .. 32. Default: 12.\n";
    std::cout << "      --maskTrigger K1 : With --maskSubjects: a window of at most K1 bits of entropy starts a segment. Default: 1.9.\n";
    std::cout << "      --maskExtend K2 : With --maskSubjects: the segment extends over adjacent windows of at most K2 bits, K1 <= K2. Default: 2.2.\n\n";
    std::cout << "   Memory\n";
    std::cout << "      --maxGpuMem val : Try not to use more than val bytes of gpu memory per gpu. Uses all available gpu memory by default\n";
    std::cout << "      --maxTempBytes val : Size of temp storage in GPU memory. Can use suffix K,M,G. Default val = " << d.memory.maxTempBytes << "\n";
    std::cout << "      --maxBatchBytes val : Process DB in batches of at most val bytes. Can use suffix K,M,G. Default val = " << d.memory.maxBatchBytes << "\n";
    std::cout << "      --maxBatchSequences val : Process DB in batches of at most val sequences. Default val = " << d.memory.maxBatchSequences << "\n\n";
    std::cout << "   Misc\n";
    std::cout << "      --dpx : Use the packed int16 / int32 kernels (the reference's DPX kernels).\n";
    std::cout << "      --refCompat : Apply gap scores -11 / -1 whatever --gop, --gex and --mat say, like the reference binary does.\n";
    std::cout << "      --of : Result output file. Parent directory must exist. Default: console output (/dev/stdout)\n";
    std::cout << "      --tsv : Print results as tab-separated values instead of plain text. \n";
    std::cout << "      --alignments : Also report where every result aligns: query and reference begin / end, alignment length, identities, gap opens and CIGAR (computed on the GPU).\n";
    std::cout << "      --pssmAlignments : --alignments for every query, --pssm queries included. Identities and the CIGAR's = / X of a PSSM are counted against the residue column of its file.\n";
    std::cout << "      --maxHsps N --hspMinScore S : With --alignments / --pssmAlignments: up to N (1 .. 16) non-overlapping local alignments per result\n"
                 "        (Waterman-Eggert: the k-th shares no aligned pair with the better ones), the further ones scoring at least S (S >= 1,\n"
                 "        needed when N > 1). TSV: one more column HSP behind CIGAR and one more line per further alignment, with its score and\n"
                 "        coordinates; plain: one more line Alignment i.k. Ranking, --maxEvalue and inclusion look at the first alignment only.\n";
    std::cout << "      --verbose : More console output. Shows timings. \n";
    std::cout << "      --printLengthPartitions : Print number of sequences per length partition in db.\n";
    std::cout << "      --interactive : Loads DB, then waits for sequence input by user\n";
    std::cout << "      --help : Print this message\n\n";
    std::cout << "   Performance and benchmarking\n";
    std::cout << "      --prefetchDBFile : Load DB into RAM immediately at program start instead of waiting for the first access.\n";
    std::cout << "      --uploadFull : If enough GPU memory is available to store full db, copy full DB to GPU before processing queries.\n";
    std::cout << "      --pseudodb num length : Use a generated DB which contains `num` equal sequences of length `length`.\n";
    std::cout << "      --singlePassType val, --manyPassType_small val, --manyPassType_large val, --overflowType val :\n";
    std::cout << "           Select kernel types for different length partitions. Valid values: Half2, DPXs16, DPXs32, Float.\n";
    std::cout << "           Misc option --dpx is equivalent to --singlePassType DPXs16 --manyPassType_small DPXs16 --manyPassType_large DPXs32 --overflowType DPXs32.\n";
    std::cout << "           Default is --singlePassType Half2 --manyPassType_small Half2 --manyPassType_large Float --overflowType Float.\n\n";
}

}  // namespace swh
