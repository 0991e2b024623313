// align — search query sequences against a DB on all visible MI355X GPUs.
// Command line, console output and result formats follow the reference (main.cu:98-426,
// SURVEY.md Appendix D); the work is done by SearchDriver through libcudasw4_amd.so.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <string_view>
#include <vector>

#include "../../../include/cudasw4_amd_msa.h"
#include "../../../include/cudasw4_amd_msa_select.h"
#include "cli_options.hpp"
#include "db_format.hpp"
#include "hit_alignment.hpp"
#include "hit_msa.hpp"
#include "pssm_build.hpp"
#include "pssm_query.hpp"
#include "search_driver.hpp"
#include "search_rank.hpp"
#include "search_stats.hpp"
#include "sequence_reader.hpp"
#include "shuffle_stats.hpp"

using namespace swh;

namespace {

// --alignments: 1-based inclusive begin / end on the query and the reference (0 when the score is 0)
struct AlignmentColumns {
    int64_t qb = 0, qe = 0, sb = 0, se = 0;
    explicit AlignmentColumns(const sw_align_result& r) {
        if (r.q_begin >= 0) {
            qb = r.q_begin + 1;
            qe = r.q_end;
            sb = r.s_begin + 1;
            se = r.s_end;
        }
    }
};

// --evalues / --maxEvalue: the fit of one query's scan and what is printed of it (nullptr: no statistics columns)
struct EvalueReport {
    SearchStats stats;
    bool filter = false;     // --maxEvalue: only results with E <= maxE are printed (none where the scan allows no fit)
    double maxE = 0;
    HitStatistics of(const ScanResult& r, const SearchDriver& d, size_t i) const {
        return hit_statistics(stats, r.scores[i], d.getReferenceLength(r.referenceIds[i]));
    }
    bool shows(const HitStatistics& h) const { return !filter || (stats.fitted() && h.e <= maxE); }
    static std::string z_text(const SearchStats& s, const HitStatistics& h) {
        if (!s.fitted()) return "*";
        char buf[48];
        std::snprintf(buf, sizeof buf, "%.2f", h.z);
        return buf;
    }
    static std::string e_text(const SearchStats& s, const HitStatistics& h) {
        if (!s.fitted()) return "*";
        char buf[48];
        std::snprintf(buf, sizeof buf, "%.3g", h.e);
        return buf;
    }
};

// --maxHsps above 1: the alignments of every result, the first one included (nullptr otherwise)
typedef HitAligner::HspLists HspLists;

// alignments: nullptr without --alignments / --pssmAlignments, else one per result
void printScanResultPlain(std::ostream& os, const ScanResult& r, const SearchDriver& d, const std::vector<HitAlignment>* alignments = nullptr,
                          const EvalueReport* ev = nullptr, const HspLists* hsps = nullptr) {
    for (size_t i = 0; i < r.scores.size(); i++) {
        const int64_t id = r.referenceIds[i];
        HitStatistics hs;
        if (ev) {
            hs = ev->of(r, d, i);
            if (!ev->shows(hs)) continue;
        }
        os << "Result " << i << ". Score: " << r.scores[i] << ". Length: " << d.getReferenceLength(id) << ". Header "
           << d.getReferenceHeader(id) << ". referenceId " << id;
        if (ev) os << " Z-score: " << EvalueReport::z_text(ev->stats, hs) << " E-value: " << EvalueReport::e_text(ev->stats, hs);
        os << "\n";
        if (alignments) {
            const HitAlignment& a = (*alignments)[i];
            const AlignmentColumns c(a.r);
            os << "Alignment " << i << ". Query " << c.qb << "-" << c.qe << ". Reference " << c.sb << "-" << c.se << ". Length "
               << a.r.columns << ". Identities " << a.r.identities << ". Gap opens " << a.r.gap_opens << ". CIGAR "
               << cigar_string(a.cigar) << "\n";
        }
        // a further alignment's Z-score and E-value: the query's fit applied to its own (non-maximal) score
        for (size_t k = 1; hsps && k < (*hsps)[i].size(); k++) {
            const HitAlignment& a = (*hsps)[i][k];
            const AlignmentColumns c(a.r);
            os << "Alignment " << i << "." << k + 1 << ". Score " << a.r.score << ". Query " << c.qb << "-" << c.qe << ". Reference " << c.sb
               << "-" << c.se << ". Length " << a.r.columns << ". Identities " << a.r.identities << ". Gap opens " << a.r.gap_opens
               << ". CIGAR " << cigar_string(a.cigar);
            if (ev) {
                const HitStatistics h = hit_statistics(ev->stats, a.r.score, d.getReferenceLength(id));
                os << " Z-score: " << EvalueReport::z_text(ev->stats, h) << " E-value: " << EvalueReport::e_text(ev->stats, h);
            }
            os << "\n";
        }
    }
}

void printTSVHeader(std::ostream& os, bool alignments, bool evalues, bool hsps = false) {
    os << "Query number\tQuery length\tQuery header\tResult number\tResult score\tReference length\tReference header\tReference ID in DB";
    if (alignments) os << "\tQuery begin\tQuery end\tReference begin\tReference end\tAlignment length\tIdentities\tGap opens\tCIGAR";
    if (hsps) os << "\tHSP";
    if (evalues) os << "\tZ-score\tE-value";
    os << "\n";
}

void printScanResultTSV(std::ostream& os, const ScanResult& r, const SearchDriver& d, int64_t queryId, int64_t queryLength,
                        std::string_view queryHeader, const std::vector<HitAlignment>* alignments = nullptr, const EvalueReport* ev = nullptr,
                        const HspLists* hsps = nullptr) {
    for (size_t i = 0; i < r.scores.size(); i++) {
        const int64_t id = r.referenceIds[i];
        HitStatistics hs;
        if (ev) {
            hs = ev->of(r, d, i);
            if (!ev->shows(hs)) continue;
        }
        os << queryId << '\t' << queryLength << '\t' << queryHeader << '\t' << i << '\t' << r.scores[i] << '\t'
           << d.getReferenceLength(id) << '\t' << d.getReferenceHeader(id) << '\t' << id;
        if (alignments) {
            const HitAlignment& a = (*alignments)[i];
            const AlignmentColumns c(a.r);
            os << '\t' << c.qb << '\t' << c.qe << '\t' << c.sb << '\t' << c.se << '\t' << a.r.columns << '\t' << a.r.identities
               << '\t' << a.r.gap_opens << '\t' << cigar_string(a.cigar);
        }
        if (hsps) os << '\t' << 1;
        if (ev) os << '\t' << EvalueReport::z_text(ev->stats, hs) << '\t' << EvalueReport::e_text(ev->stats, hs);
        os << "\n";
        // every further alignment: the result's line again with that alignment's score, coordinates and statistics (the
        // query's fit applied to its own, non-maximal, score)
        for (size_t k = 1; hsps && k < (*hsps)[i].size(); k++) {
            const HitAlignment& a = (*hsps)[i][k];
            const AlignmentColumns c(a.r);
            os << queryId << '\t' << queryLength << '\t' << queryHeader << '\t' << i << '\t' << a.r.score << '\t'
               << d.getReferenceLength(id) << '\t' << d.getReferenceHeader(id) << '\t' << id << '\t' << c.qb << '\t' << c.qe << '\t'
               << c.sb << '\t' << c.se << '\t' << a.r.columns << '\t' << a.r.identities << '\t' << a.r.gap_opens << '\t'
               << cigar_string(a.cigar) << '\t' << k + 1;
            if (ev) {
                const HitStatistics h = hit_statistics(ev->stats, a.r.score, d.getReferenceLength(id));
                os << '\t' << EvalueReport::z_text(ev->stats, h) << '\t' << EvalueReport::e_text(ev->stats, h);
            }
            os << "\n";
        }
    }
}

struct Stopwatch {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void print(const char* label) const {
        std::cout << "# elapsed time (" << label << "): " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << "s\n";
    }
};

void reportScan(const ProgramOptions& o, const ScanResult& r) {
    if (o.verbose) std::cout << "Done. Scan time: " << r.stats.seconds << " s, " << r.stats.gcups << " GCUPS\n";
    else std::cout << "Done.\n";
}

// --statistics shuffled: the calibrator and the calibration of the query in flight (one at a time).  Every query, and every
// round's PSSM, is calibrated right before it is submitted; under --rankBy evalue the driver ranks it by that fit.
struct ShuffledStatistics {
    std::unique_ptr<ShuffleCalibrator> calibrator;
    SearchStats current;
    void finish(SearchDriver& driver, const std::unique_ptr<Calibration>& c, bool ranked) {
        current = c->stats;
        if (ranked) {
            RankFit f;
            f.ok = current.fitted(); f.a = current.a; f.b1 = current.b1; f.sd = current.sd;
            driver.setRankFit(&f);
        }
    }
    void beforeSubmit(SearchDriver& driver, const char* letters, int32_t qlen, bool ranked) { finish(driver, calibrator->calibrate(letters, qlen), ranked); }
    void beforeSubmit(SearchDriver& driver, const int8_t* pssm, int32_t qlen, bool ranked) { finish(driver, calibrator->calibrate(pssm, qlen), ranked); }
};
ShuffledStatistics* shuffled = nullptr;   // (non-null under --statistics shuffled)

// --outMsa: the query-anchored MSA of one query's reported results (hit_msa.hpp).  The aligner holds the
// results' alignments of the query's last round on the device (already made for --alignments or by the last round's PSSM
// build; made here otherwise); the filter runs there, the writer on the host.
struct MsaOutput {
    HitAligner* aligner = nullptr;
    std::unique_ptr<HitMsa> msa;
    // master: the query's letters (a PSSM query: the residue column of its file); pssm: what the results were scanned with
    // (nullptr: the letters); alignments: nullptr when nothing has aligned the results yet
    void write(const ProgramOptions& o, const SearchDriver& d, int64_t queryNum, std::string_view queryHeader, const std::string& master,
               const int8_t* pssm, const ScanResult& r, const std::vector<HitAlignment>* alignments, const EvalueReport* ev) {
        const int32_t qlen = int32_t(master.size());
        std::vector<HitAlignment> own;
        if (!alignments) {
            own = pssm ? aligner->align(pssm, qlen, master.data(), r) : aligner->align(master.data(), qlen, r);
            alignments = &own;
        }
        const size_t n = r.scores.size();
        std::vector<uint8_t> shown(n, 1);   // (--maxEvalue: the results that are printed)
        size_t reported = 0, noTrace = 0;
        for (size_t i = 0; i < n; i++) {
            shown[i] = !ev || ev->shows(ev->of(r, d, i));
            reported += shown[i];
            noTrace += shown[i] && (*alignments)[i].r.status == SW_ALIGN_NO_TRACE;
        }
        std::vector<uint8_t> keep(n, 0);
        int32_t purged = 0;
        int32_t counts[4] = {0, 0, 0, 0};
        if (o.selectsMsaRows()) {
            if (n > 0) {
                MsaSelectParams params;
                params.minCoverage = o.msaMinCoverage;
                params.minQueryIdentity = o.msaMinQueryIdentity;
                params.diff = o.msaDiff;
                params.ladder = o.msaLadder;
                const MsaSelectResult f = msa->select(master.data(), qlen, shown.data(), params, false);
                for (size_t i = 0; i < n; i++) keep[i] = f.state[i] == SW_MSA_STATE_KEPT;
                std::copy(f.counts, f.counts + 4, counts);
            }
        } else if (n > 0) {
            const MsaFilterResult f = msa->filter(master.data(), qlen, shown.data(), o.msaMaxIdentity, false);
            keep.assign(f.keep.begin(), f.keep.begin() + long(n));
            purged = f.purged;
        }
        std::vector<std::string> headers(n), letters(n);
        for (size_t i = 0; i < n; i++)
            if (keep[i]) {
                headers[i] = std::string(d.getReferenceHeader(r.referenceIds[i]));
                letters[i] = d.getReferenceSequence(r.referenceIds[i]);
            }
        MsaFormat format = MsaFormat::A3m;
        parse_msa_format(o.msaFormat, format);
        const std::string path = o.outMsa + "." + std::to_string(queryNum) + (format == MsaFormat::A3m ? ".a3m" : ".fasta");
        std::string header(queryHeader);
        if (!header.empty() && header[0] == '>') header.erase(0, 1);
        const size_t written = write_msa(path, format, master, header, headers, letters, *alignments, keep.data());
        if (o.verbose && o.selectsMsaRows())
            std::cout << "msa: " << written << " of " << reported << " results written, " << counts[1] << " below coverage, " << counts[2]
                      << " below query identity, " << counts[3] << " thinned, " << noTrace << " without a trace\n";
        else if (o.verbose)
            std::cout << "msa: " << written << " of " << reported << " results written, " << purged << " purged, " << noTrace
                      << " without a trace\n";
    }
};
MsaOutput* msaOut = nullptr;   // (non-null under --outMsa)

// the fit of a scan made with the statistics on (--evalues / --maxEvalue / --inclusionEvalue): of the scan's own table, or
// under --statistics shuffled the query's calibration with N from the scan's table
SearchStats fitOf(const ScanResult& r) {
    if (r.table.empty()) throw std::runtime_error("internal error: a scan without its score table");
    if (shuffled) return calibrated_stats(shuffled->current, table_count(r.table.front()));
    return stats_from_table(r.table.front());
}

void reportStatistics(const ProgramOptions& o, const SearchStats& s) {
    if (!o.verbose) return;
    std::cout << "statistics: ";
    if (shuffled) std::cout << "shuffled " << shuffled->calibrator->subjects() << " subjects x " << shuffled->calibrator->replicas() << ", ";
    if (!s.fitted()) std::cout << "no fit\n";
    else std::cout << "N " << s.N << " fitted on " << s.nIncluded << " a " << s.a << " b " << s.b1 << " sd " << s.sd
                   << " rounds " << s.rounds << "\n";
}

// what the result lines of a query print of its statistics: nullptr without --evalues / --maxEvalue
const EvalueReport* evalueReport(const ProgramOptions& o, const ScanResult& r, EvalueReport& storage) {
    if (!o.wantStatistics()) return nullptr;
    storage.stats = fitOf(r);
    storage.filter = o.haveMaxEvalue;
    storage.maxE = o.maxEvalue;
    reportStatistics(o, storage.stats);
    return o.reportEvalues() ? &storage : nullptr;
}

// --rankBy evalue --maxEvalue X --verbose: how many subjects of the whole DB lie at or under the threshold, and how many of
// them the --top list reports
// --verbose with --maskSubjects: what the pass over the DB behind the query collected last masked
void reportMasking(const ProgramOptions& o, const SearchDriver& d) {
    if (!o.verbose || !d.masksSubjects()) return;
    const SearchDriver::MaskingCounts c = d.maskingCounts();
    std::cout << "subject masking: window " << d.maskParams().window << " trigger " << o.maskTrigger << " extend " << o.maskExtend << ": "
              << c.positions << " of " << c.residuesSeen << " residues in " << c.subjects << " of " << d.numSequences() << " subjects\n";
}

void reportSignificant(const ProgramOptions& o, const ScanResult& r, const SearchDriver& d, const EvalueReport* ev) {
    if (!o.verbose || !o.rankByEvalue() || !o.haveMaxEvalue || !(o.maxEvalue > 0) || !ev) return;
    if (r.significant < 0) { std::cout << "significant: no fit\n"; return; }
    size_t reported = 0;
    for (size_t i = 0; i < r.scores.size(); i++) reported += ev->shows(ev->of(r, d, i)) ? 1 : 0;
    std::cout << "significant: " << r.significant << " subjects at E <= " << o.maxEvalue << " (" << reported << " reported)\n";
}

// --iterations / --outPssm: the rounds of one query behind its first scan (pssm_build.hpp; DESIGN.md "Building a PSSM").
struct IterationResult {
    std::vector<int8_t> built;              // the PSSM built from the last round's results
    std::vector<HitAlignment> alignments;   // the last round's results aligned against that round's scoring
    HspLists hsps;                          // --maxHsps above 1: all alignments of those results (element 0 = `alignments`)
};

// --maxHsps above 1: all alignments of every result.  pssm: what the results were scanned with (nullptr: `letters`, which
// are then the query; else `letters` are the consensus).  The first alignments (what is printed without --maxHsps) are element
// 0 of every list and replace `first`.
HspLists alignHsps(const ProgramOptions& o, HitAligner& aligner, const std::string& letters, const int8_t* pssm, const ScanResult& r,
                   std::vector<HitAlignment>& first) {
    const int32_t qlen = int32_t(letters.size());
    HspLists lists = pssm ? aligner.align(pssm, qlen, letters.data(), r, o.maxHsps, o.hspMinScore)
                          : aligner.align(letters.data(), qlen, r, o.maxHsps, o.hspMinScore);
    first.resize(lists.size());
    for (size_t i = 0; i < lists.size(); i++) first[i] = lists[i].front();
    return lists;
}

// master: the query's letters (a PSSM input: the residue column of its file); first: the PSSM of round 1, or nullptr (the
// letters).  r: in, the results of round 1; out, those of the last round.  Every round builds a PSSM from its results; round
// k + 1 scans with the one of round k.  Stops after --iterations rounds, or when a round includes the ids the round before
// included.
IterationResult runIterations(const ProgramOptions& o, SearchDriver& driver, PssmBuilder& builder, int64_t queryNum, const std::string& master,
                              const int8_t* first, ScanResult& r) {
    const int32_t qlen = int32_t(master.size());
    std::vector<int8_t> scoring;
    if (first) scoring.assign(first, first + size_t(qlen) * kPssmColumns);
    std::vector<int64_t> previous;
    IterationResult out;
    for (int round = 1;; round++) {
        PssmBuildInfo info;
        // --inclusionEvalue: a result goes in by its E-value under THIS round's fit (none where the scan allows no fit)
        std::vector<uint8_t> admitted;
        if (o.haveInclusionEvalue) {
            const SearchStats st = fitOf(r);
            admitted.resize(r.scores.size());
            for (size_t i = 0; i < r.scores.size(); i++)
                admitted[i] = st.fitted() && hit_statistics(st, r.scores[i], driver.getReferenceLength(r.referenceIds[i])).e <= o.inclusionEvalue;
        }
        out.built = builder.build(master.data(), qlen, scoring.empty() ? nullptr : scoring.data(), r.referenceIds.data(),
                                  r.scores.data(), r.scores.size(), o.inclusionScore, o.pseudocount, &info,
                                  o.haveInclusionEvalue ? admitted.data() : nullptr, o.reportAlignments() ? o.maxHsps : 1, o.hspMinScore,
                                  o.purgeIdentity);
        out.alignments = std::move(info.alignments);
        out.hsps = std::move(info.hsps);
        std::vector<int64_t> included;
        for (size_t i = 0; i < info.included.size(); i++)
            if (info.included[i]) included.push_back(r.referenceIds[i]);
        std::sort(included.begin(), included.end());
        const bool converged = round > 1 && included == previous;
        if (o.verbose)
            std::cout << "Query " << queryNum << " round " << round << ": " << r.scores.size() << " results, " << info.used
                      << " in the PSSM, " << info.belowScore << (o.haveInclusionEvalue ? " above the inclusion E-value, " : " below the inclusion score, ")
                      << info.noTrace << " without a trace, "
                      << info.copies << " copies of the query"
                      << (o.havePurgeIdentity ? ", " + std::to_string(info.purged) + " purged as redundant" : std::string())
                      << ", lambda " << info.lambda
                      << (converged && round < o.iterations ? ", converged" : "") << "\n";
        if (round >= o.iterations || converged) break;
        previous = std::move(included);
        scoring = out.built;
        if (shuffled) shuffled->beforeSubmit(driver, scoring.data(), qlen, o.rankByEvalue());
        submit_pssm(driver, scoring.data(), qlen);
        r = driver.collect();
    }
    if (!o.outPssm.empty()) {
        std::string consensus = master;
        for (char& c : consensus)
            if (!(std::isalpha((unsigned char)c) || c == '*' || c == '-')) c = 'X';
        write_ascii_pssm(o.outPssm + "." + std::to_string(queryNum) + ".pssm", out.built.data(), qlen, consensus);
    }
    return out;
}

// All queries of a file (main.cu:217-260), one at a time like the reference — unless the DB's shards are small enough for
// the tail hand-over (SearchDriver::prefersTwoInFlight: resident shards of a few rounds of workgroups, or a query that is
// scanned in a few milliseconds; the next query's launch fills the slots the current one's last round leaves idle: +4 %
// on 125 000 subjects, +26 % for a stream of 48-residue queries on a Swiss-Prot-sized DB): then, and with
// CUDASW4_AMD_PIPELINE=1, the next query is submitted before the current one is collected (SearchDriver::submit /
// collect).  On large DBs two queries in flight bring nothing (10^6 subjects) or cost (-0.8 % on a Swiss-Prot-like one);
// CUDASW4_AMD_PIPELINE=0 keeps one query at a time everywhere.  Output order and format are the reference's either way; a
// query's line is printed when its results are in.
// aligner: non-null with --alignments / --pssmAlignments (every query's hits are aligned right after its collect, against that query)
void processQueryFile(const std::string& file, const ProgramOptions& o, SearchDriver& driver, std::ostream& out, bool interactive,
                      HitAligner* aligner, PssmBuilder* iteration = nullptr) {
    SequenceReader reader(file);
    struct Pending { int64_t num; std::string header, sequence; };
    std::deque<Pending> pending;
    int64_t query_num = 0;
    const char* pipe = std::getenv("CUDASW4_AMD_PIPELINE");
    // how many queries may be pending once a query of this length has been submitted
    auto max_in_flight = [&](size_t queryLength) {
        if (iteration) return 1;   // the rounds of a query are scans of their own: nothing else may be in flight
        if (o.rankByEvalue()) return 1;   // the second half of a ranked query reads its score array again (SearchDriver::setRanking)
        if (shuffled) return 1;           // one calibration at a time
        if (pipe) return pipe[0] == '1' ? 2 : 1;
        return driver.preferredInFlight(int32_t(std::min<size_t>(queryLength, size_t(INT32_MAX))));
    };
    if (!interactive) driver.totalTimerStart();
    auto finish_oldest = [&]() {
        const Pending q = std::move(pending.front());
        pending.pop_front();
        std::cout << "Processing query " << q.num << " ... ";
        std::cout.flush();
        ScanResult r = driver.collect();
        reportScan(o, r);
        reportMasking(o, driver);
        IterationResult rounds;
        if (iteration) rounds = runIterations(o, driver, *iteration, q.num, q.sequence, nullptr, r);
        if (o.numTopOutputs > 0 || interactive) {
            std::vector<HitAlignment> alignments;
            HspLists lists;
            if (iteration && (aligner || msaOut)) {
                alignments = std::move(rounds.alignments);
                lists = std::move(rounds.hsps);
            } else if (aligner && o.reportHsps()) lists = alignHsps(o, *aligner, q.sequence, nullptr, r, alignments);
            else if (aligner) alignments = aligner->align(q.sequence.data(), int32_t(q.sequence.size()), r);
            const std::vector<HitAlignment>* al = aligner ? &alignments : nullptr;
            const HspLists* hsps = aligner && o.reportHsps() ? &lists : nullptr;
            EvalueReport evStorage;
            const EvalueReport* ev = evalueReport(o, r, evStorage);
            if (o.outputMode == ProgramOptions::OutputMode::Plain) {
                (interactive ? std::cout : out) << "Query " << q.num << ", header" << q.header << ", length " << q.sequence.size()
                                                << ", num overflows " << r.stats.numOverflows << "\n";
                printScanResultPlain(out, r, driver, al, ev, hsps);
            } else {
                printScanResultTSV(out, r, driver, interactive ? -1 : q.num, int64_t(q.sequence.size()), interactive ? "-" : q.header, al, ev, hsps);
            }
            out.flush();
            reportSignificant(o, r, driver, ev);
            if (msaOut && !interactive)
                msaOut->write(o, driver, q.num, q.header, q.sequence, nullptr, r, aligner || iteration ? &alignments : nullptr, ev);
        }
    };
    try {
        while (reader.next()) {
            pending.push_back(Pending{query_num++, reader.header(), reader.sequence()});
            if (shuffled) shuffled->beforeSubmit(driver, pending.back().sequence.data(), int32_t(pending.back().sequence.size()), o.rankByEvalue());
            driver.submit(pending.back().sequence.data(), int32_t(pending.back().sequence.size()));
            const int maxInFlight = max_in_flight(pending.back().sequence.size());
            while (driver.inFlight() >= maxInFlight) finish_oldest();
        }
        while (driver.inFlight() > 0) finish_oldest();
    } catch (...) {
        while (driver.inFlight() > 0) {  // leave the driver usable (interactive mode goes on after an error)
            try { (void)driver.collect(); } catch (...) {}
        }
        throw;
    }
    if (!interactive) {
        const BenchmarkStats total = driver.totalTimerStop();
        if (o.verbose) std::cout << "Total time: " << total.seconds << " s, " << total.gcups << " GCUPS\n";
    }
}

// One --pssm file: a single query (number 0 of its "file"), printed like a query of a query file; header = the file's base name
// aligner: non-null with --pssmAlignments (the hits are aligned against the PSSM; '=' / 'X' against the file's residue column)
void processPssmQuery(const PssmQuery& q, const ProgramOptions& o, SearchDriver& driver, std::ostream& out, HitAligner* aligner,
                      PssmBuilder* iteration = nullptr) {
    driver.totalTimerStart();
    std::cout << "Processing query " << 0 << " ... ";
    std::cout.flush();
    if (shuffled) shuffled->beforeSubmit(driver, q.scores.data(), q.length(), o.rankByEvalue());
    submit_pssm(driver, q.scores.data(), q.length());
    ScanResult r = driver.collect();
    reportScan(o, r);
    reportMasking(o, driver);
    IterationResult rounds;
    if (iteration) rounds = runIterations(o, driver, *iteration, 0, q.consensus, q.scores.data(), r);
    if (o.numTopOutputs > 0) {
        std::vector<HitAlignment> alignments;
        HspLists lists;
        if (iteration && (aligner || msaOut)) {
            alignments = std::move(rounds.alignments);
            lists = std::move(rounds.hsps);
        } else if (aligner && o.reportHsps()) lists = alignHsps(o, *aligner, q.consensus, q.scores.data(), r, alignments);
        else if (aligner) alignments = aligner->align(q.scores.data(), q.length(), q.consensus.data(), r);
        const std::vector<HitAlignment>* al = aligner ? &alignments : nullptr;
        const HspLists* hsps = aligner && o.reportHsps() ? &lists : nullptr;
        EvalueReport evStorage;
        const EvalueReport* ev = evalueReport(o, r, evStorage);
        if (o.outputMode == ProgramOptions::OutputMode::Plain) {
            out << "Query " << 0 << ", header " << q.name << ", length " << q.length() << ", num overflows " << r.stats.numOverflows << "\n";
            printScanResultPlain(out, r, driver, al, ev, hsps);
        } else {
            printScanResultTSV(out, r, driver, 0, int64_t(q.length()), q.name, al, ev, hsps);
        }
        out.flush();
        reportSignificant(o, r, driver, ev);
        // (after the last round the results were scanned with the PSSM of the round before: the last build's alignments are
        // against it; without rounds they are against the file's PSSM)
        if (msaOut)
            msaOut->write(o, driver, 0, q.name, q.consensus, q.scores.data(), r, aligner || iteration ? &alignments : nullptr, ev);
    }
    const BenchmarkStats total = driver.totalTimerStop();
    if (o.verbose) std::cout << "Total time: " << total.seconds << " s, " << total.gcups << " GCUPS\n";
}

}  // namespace

int main(int argc, char** argv) {
    ProgramOptions options;
    const bool ok = parseArgs(argc, argv, options);
    if (!ok || options.help) {
        printHelp(argv);
        return 0;
    }
    printOptions(options);
    try {
        // PSSM queries are read and validated before any device is opened: a malformed file is an error of the command line
        if (!options.pssmFiles.empty() && options.alignments && !options.pssmAlignments)
            throw std::runtime_error("--pssm cannot be combined with --alignments: use --pssmAlignments to align the results of every query, PSSM queries included");
        if (!options.pssmFiles.empty() && options.interactive)
            throw std::runtime_error("--pssm cannot be combined with --interactive");
        if ((options.haveMaxHsps || options.haveHspMinScore) && !options.reportAlignments())
            throw std::runtime_error("--maxHsps / --hspMinScore need --alignments or --pssmAlignments: they say how many alignments of a result are reported");
        if (options.maxHsps < 1 || options.maxHsps > 16) throw std::runtime_error("--maxHsps must lie in 1 .. 16");
        if (options.haveHspMinScore && options.hspMinScore < 1) throw std::runtime_error("--hspMinScore must be at least 1");
        if (options.maxHsps > 1 && !options.haveHspMinScore)
            throw std::runtime_error("--maxHsps above 1 needs --hspMinScore S: further alignments of a result are reported down to the raw score S");
        if (options.iterations < 1) throw std::runtime_error("--iterations must be at least 1");
        if (options.haveInclusionScore && options.haveInclusionEvalue)
            throw std::runtime_error("--inclusionScore and --inclusionEvalue cannot be combined: results go into the PSSM by one rule");
        if (options.buildsPssm() && !options.haveInclusionScore && !options.haveInclusionEvalue)
            throw std::runtime_error("--iterations above 1 and --outPssm need --inclusionScore S (results go into the PSSM by raw score, "
                                     "at least S) or --inclusionEvalue X (by their E-values, at most X)");
        if (options.rankBy != "score" && options.rankBy != "evalue")
            throw std::runtime_error("--rankBy must be score or evalue, not '" + options.rankBy + "'");
        if (options.statistics != "scan" && options.statistics != "shuffled")
            throw std::runtime_error("--statistics must be scan or shuffled, not '" + options.statistics + "'");
        if ((options.haveShuffles || options.haveShuffleSubjects || options.haveShuffleSeed) && !options.shuffledStatistics())
            throw std::runtime_error("--shuffles / --shuffleSubjects / --shuffleSeed need --statistics shuffled: they say what the statistics are calibrated on");
        if (options.haveShuffles && (options.shuffles < 1 || options.shuffles > kShuffleMaxReplicas)) throw std::runtime_error("--shuffles must lie in 1 .. 64");
        if (options.haveShuffleSubjects && (options.shuffleSubjects < 1 || options.shuffleSubjects > INT32_MAX))
            throw std::runtime_error("--shuffleSubjects must be at least 1");
        if (options.haveShuffleSeed && options.shuffleSeed > UINT32_MAX) throw std::runtime_error("--shuffleSeed must lie in 0 .. 4294967295");
        if (options.shuffledStatistics() && options.interactive) throw std::runtime_error("--statistics shuffled cannot be combined with --interactive");
        if (options.haveMaxEvalue && !(options.maxEvalue >= 0)) throw std::runtime_error("--maxEvalue must not be negative");
        if (options.haveInclusionEvalue && !(options.inclusionEvalue >= 0)) throw std::runtime_error("--inclusionEvalue must not be negative");
        if (options.wantStatistics() && options.interactive) throw std::runtime_error("--evalues / --maxEvalue / --inclusionEvalue / --rankBy evalue cannot be combined with --interactive");
        if (!(options.pseudocount > 0)) throw std::runtime_error("--pseudocount must be positive");
        if (options.buildsPssm() && options.interactive) throw std::runtime_error("--iterations / --outPssm cannot be combined with --interactive");
        if (options.buildsPssm() && options.numTopOutputs < 1) throw std::runtime_error("--iterations / --outPssm need --top of at least 1: the PSSM is built from the reported results");
        {
            auto percent = [](const std::string& text, const char* flag) {
                size_t used = 0;
                long v = 0;
                try { v = std::stol(text, &used); } catch (...) { used = 0; }
                if (text.empty() || used != text.size() || v < 1 || v > 100)
                    throw std::runtime_error(std::string(flag) + " must be an integer in 1 .. 100, not '" + text + "'");
                return int(v);
            };
            if ((options.haveMsaFormat || options.haveMsaMaxIdentity) && !options.haveOutMsa)
                throw std::runtime_error("--msaFormat / --msaMaxIdentity need --outMsa PREFIX: they say how the multiple alignment is written");
            if (options.selectsMsaRows() && !options.haveOutMsa)
                throw std::runtime_error("--msaMinCoverage / --msaMinQueryIdentity / --msaDiff / --msaDiffLadder need --outMsa PREFIX: they say which results the multiple alignment keeps");
            if (options.haveOutMsa && options.outMsa.empty()) throw std::runtime_error("--outMsa needs a file prefix");
            MsaFormat format;
            if (!parse_msa_format(options.msaFormat, format))
                throw std::runtime_error("--msaFormat must be a3m or fasta, not '" + options.msaFormat + "'");
            if (options.haveMsaMaxIdentity) options.msaMaxIdentity = percent(options.msaMaxIdentityText, "--msaMaxIdentity");
            if (options.havePurgeIdentity) options.purgeIdentity = percent(options.purgeIdentityText, "--purgeIdentity");
            if (options.haveMsaMinCoverage) options.msaMinCoverage = percent(options.msaMinCoverageText, "--msaMinCoverage");
            if (options.haveMsaMinQueryIdentity) options.msaMinQueryIdentity = percent(options.msaMinQueryIdentityText, "--msaMinQueryIdentity");
            if (options.haveMsaDiff) {
                const std::string& text = options.msaDiffText;
                size_t used = 0;
                long v = 0;
                try { v = std::stol(text, &used); } catch (...) { used = 0; }
                if (text.empty() || used != text.size() || v < 1 || v > INT32_MAX)
                    throw std::runtime_error("--msaDiff must be an integer of at least 1, not '" + text + "'");
                options.msaDiff = int(v);
            }
            if (options.haveMsaDiffLadder) {
                if (!options.haveMsaDiff) throw std::runtime_error("--msaDiffLadder needs --msaDiff D: it names the rungs of the diversity selection");
                if (options.haveMsaMaxIdentity)
                    throw std::runtime_error("--msaDiffLadder cannot be combined with --msaMaxIdentity: the ladder's last rung is the identity cut");
                const std::string& text = options.msaDiffLadderText;
                const std::string bad = "--msaDiffLadder must be 1 .. 16 strictly ascending integers in 1 .. 100 separated by commas, not '" + text + "'";
                for (size_t at = 0; at <= text.size();) {
                    const size_t comma = std::min(text.find(',', at), text.size());
                    const std::string part = text.substr(at, comma - at);
                    size_t used = 0;
                    long v = 0;
                    try { v = std::stol(part, &used); } catch (...) { used = 0; }
                    if (part.empty() || used != part.size() || v < 1 || v > 100) throw std::runtime_error(bad);
                    if (!options.msaLadder.empty() && v <= options.msaLadder.back()) throw std::runtime_error(bad);
                    options.msaLadder.push_back(int32_t(v));
                    at = comma + 1;
                }
                if (options.msaLadder.size() > SW_MSA_SELECT_MAX_LADDER) throw std::runtime_error(bad);
            } else if (options.haveMsaDiff) {   // 20, 30, ... below P, then P
                const int last = options.haveMsaMaxIdentity ? options.msaMaxIdentity : 90;
                for (int rung = 20; rung < last; rung += 10) options.msaLadder.push_back(rung);
                options.msaLadder.push_back(last);
            } else if (options.selectsMsaRows()) {
                // coverage / query identity alone: the weakest cut the selection has (a result whose every residue repeats a
                // written row), unless --msaMaxIdentity names one
                options.msaLadder.push_back(options.haveMsaMaxIdentity ? options.msaMaxIdentity : 100);
            }
            if (options.havePurgeIdentity && !options.buildsPssm())
                throw std::runtime_error("--purgeIdentity needs --iterations above 1 or --outPssm: it says which results go into the PSSM");
            if ((options.haveOutMsa || options.havePurgeIdentity) && options.interactive)
                throw std::runtime_error("--outMsa / --msaFormat / --msaMaxIdentity / --purgeIdentity cannot be combined with --interactive");
            if (options.haveOutMsa && options.numTopOutputs < 1)
                throw std::runtime_error("--outMsa needs --top of at least 1: the alignment is made of the reported results");
            if (options.haveOutMsa && options.numTopOutputs > SW_MSA_MAX_HITS)
                throw std::runtime_error("--outMsa takes --top up to " + std::to_string(SW_MSA_MAX_HITS));
            if (options.selectsMsaRows() && options.numTopOutputs > SW_MSA_SELECT_MAX_HITS)
                throw std::runtime_error("--msaMinCoverage / --msaMinQueryIdentity / --msaDiff take --top up to " + std::to_string(SW_MSA_SELECT_MAX_HITS));
        }
        if ((options.haveMaskWindow || options.haveMaskTrigger || options.haveMaskExtend) && !options.maskSubjects)
            throw std::runtime_error("--maskWindow / --maskTrigger / --maskExtend need --maskSubjects: they say how the subjects are masked");
        MaskParams maskParams;
        if (options.maskSubjects) {
            auto number = [](const std::string& text, const char* flag, bool integer) {
                char* end = nullptr;
                const double v = integer ? double(std::strtol(text.c_str(), &end, 10)) : std::strtod(text.c_str(), &end);
                if (text.empty() || *end != 0 || !std::isfinite(v)) throw std::runtime_error(std::string(flag) + " needs a number, not '" + text + "'");
                return v;
            };
            const double window = number(options.maskWindow, "--maskWindow", true);
            const double trigger = number(options.maskTrigger, "--maskTrigger", false), extend = number(options.maskExtend, "--maskExtend", false);
            if (window < 4 || window > 32) throw std::runtime_error("--maskWindow must lie in 4 .. 32");
            if (trigger > extend) throw std::runtime_error("--maskTrigger must not be above --maskExtend: a segment starts at a window of at most K1 bits and extends over windows of at most K2");
            maskParams = mask_params_from_bits(int(window), trigger, extend);
        }
        std::vector<PssmQuery> pssmQueries;
        for (const auto& file : options.pssmFiles) pssmQueries.push_back(read_ascii_pssm(file));
        std::vector<int> deviceIds;
        int num = 0;
        if (hipGetDeviceCount(&num) != hipSuccess) num = 0;
        for (int i = 0; i < num; i++) deviceIds.push_back(i);
        if (deviceIds.empty()) throw std::runtime_error("No GPU found");
        if (options.verbose) {
            std::cout << "Will use GPU";
            for (int x : deviceIds) std::cout << " " << x;
            std::cout << "\n";
        }
        if (deviceIds.size() == 1) {
            // one GPU: this thread issues everything (with several, every GPU has a worker thread on its own node): run it
            // on the CPUs next to the GPU (CUDASW4_AMD_NO_NUMA_BIND=1: leave the affinity alone)
            const char* no = std::getenv("CUDASW4_AMD_NO_NUMA_BIND");
            const int node = numa_node_of_device(deviceIds[0]);
            if (!(no && no[0] == '1') && bind_thread_to_numa_node(node) && options.verbose)
                std::cout << "GPU " << deviceIds[0] << " is on NUMA node " << node << ": host threads bound to it\n";
        }
        std::ofstream outputfile(options.outputfile);
        if (!outputfile) throw std::runtime_error("Cannot open file " + options.outputfile);
        if (options.outputMode == ProgramOptions::OutputMode::TSV) printTSVHeader(outputfile, options.reportAlignments(), options.reportEvalues(), options.reportHsps());

        SearchDriver driver(deviceIds, options.numTopOutputs, options.matrix, options.kernels, options.memory, options.verbose,
                            options.effectiveGop(), options.effectiveGex());
        if (options.maskSubjects) enable_subject_masking(driver, &maskParams);
        if (!options.usePseudoDB) {
            if (options.verbose) std::cout << "Reading Database: \n";
            Stopwatch t;
            bool mapped = true;
            auto db = Database::open_or_read(options.dbPrefix, options.prefetchDBFile, &mapped);
            if (options.verbose && !mapped) std::cout << "Failed to map db files. Using fallback db.\n";  // main.cu:180-183
            if (options.verbose) t.print("Read DB");
            driver.setDatabase(db);
        } else {
            if (options.verbose) std::cout << "Generating pseudo db\n";
            Stopwatch t;
            auto db = Database::pseudo(size_t(options.pseudoDBSize), options.pseudoDBLength);
            if (options.verbose) t.print("Generate DB");
            driver.setDatabase(db);
        }
        if (options.verbose) {
            driver.printDBInfo();
            if (options.printLengthPartitions) driver.printDBLengthPartitions();
        }
        if (options.loadFullDBToGpu) driver.prefetchDBToGpus();
        if (options.wantStatistics()) enable_statistics(driver, true);
        if (options.rankByEvalue()) set_ranking(driver, true, options.haveMaxEvalue ? options.maxEvalue : 0.0);
        ShuffledStatistics shuffledStorage;
        if (options.shuffledStatistics()) {
            shuffledStorage.calibrator = std::make_unique<ShuffleCalibrator>(driver, int32_t(options.shuffleSubjects), int32_t(options.shuffles),
                                                                             uint32_t(options.shuffleSeed));
            shuffled = &shuffledStorage;
        }
        std::unique_ptr<HitAligner> aligner;
        if (options.reportAlignments() || options.buildsPssm() || options.writesMsa()) aligner = std::make_unique<HitAligner>(driver);
        std::unique_ptr<PssmBuilder> iteration;   // (non-null: every query goes through its rounds)
        if (options.buildsPssm()) iteration = std::make_unique<PssmBuilder>(driver, *aligner);
        HitAligner* const reporting = options.reportAlignments() ? aligner.get() : nullptr;   // (alignments are printed)
        MsaOutput msaStorage;
        if (options.writesMsa()) {
            msaStorage.aligner = aligner.get();
            msaStorage.msa = std::make_unique<HitMsa>(*aligner);
            msaOut = &msaStorage;
        }

        if (!options.interactive) {
            size_t nextPssm = 0;
            for (const auto& input : options.inputs) {
                std::cout << "Processing query file " << input.path << "\n";
                if (input.pssm) processPssmQuery(pssmQueries[nextPssm++], options, driver, outputfile, reporting, iteration.get());
                else processQueryFile(input.path, options, driver, outputfile, false, reporting, iteration.get());
            }
        } else {
            // main.cu:336-424
            std::cout << "Interactive mode ready\n";
            std::cout << "Use 's inputsequence' to query inputsequence against the database. Press ENTER twice to begin.\n";
            std::cout << "Use 'f inputfile' to query all sequences in inputfile\n";
            std::cout << "Use 'exit' to terminate\n";
            std::cout << "Waiting for command...\n";
            std::string line;
            while (std::getline(std::cin, line)) {
                std::stringstream ss(line);
                std::string command, argument;
                ss >> command;
                if (command.empty()) continue;
                if (command == "exit") break;
                if (command == "s") {
                    if (ss >> argument) {
                        std::string sequence = argument;
                        while (std::getline(std::cin, line)) {
                            if (line.empty()) break;
                            sequence += line;
                        }
                        std::cout << "sequence: " << sequence << "\n";
                        std::cout << "Processing query " << 0 << " ... ";
                        std::cout.flush();
                        ScanResult r = driver.scan(sequence.data(), int32_t(sequence.size()));
                        reportScan(options, r);
                        reportMasking(options, driver);
                        std::vector<HitAlignment> alignments;
                        HspLists lists;
                        if (aligner && options.reportHsps()) lists = alignHsps(options, *aligner, sequence, nullptr, r, alignments);
                        else if (aligner) alignments = aligner->align(sequence.data(), int32_t(sequence.size()), r);
                        const std::vector<HitAlignment>* al = aligner ? &alignments : nullptr;
                        const HspLists* hsps = aligner && options.reportHsps() ? &lists : nullptr;
                        if (options.outputMode == ProgramOptions::OutputMode::Plain) printScanResultPlain(outputfile, r, driver, al, nullptr, hsps);
                        else printScanResultTSV(outputfile, r, driver, -1, int64_t(sequence.size()), "-", al, nullptr, hsps);
                        outputfile.flush();
                    } else {
                        std::cout << "Missing argument for command 's'\n";
                    }
                } else if (command == "f") {
                    if (ss >> argument) {
                        try {
                            processQueryFile(argument, options, driver, outputfile, true, aligner.get());
                        } catch (...) {
                            std::cout << "Error\n";
                        }
                    } else {
                        std::cout << "Missing argument for command 'f' \n";
                    }
                } else {
                    std::cout << "Unrecognized command: " << command << "\n";
                }
                std::cout << "Waiting for command...\n";
            }
        }
    } catch (const std::exception& e) {
        std::cerr << "align: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
