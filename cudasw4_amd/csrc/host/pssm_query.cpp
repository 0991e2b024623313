// pssm_query.cpp — PSSM queries of the host driver: ASCII reader, submit, and the C entry points swdrv_scan_pssm /
// swdrv_scan_submit_pssm.
//
// Kept out of search_driver.cpp and driver_capi.cpp on purpose (like hit_alignment.cpp): tests/host/fake_gpu links exactly
// those files against a fake of the C ABI that has no sw_set_query_pssm.  The driver reaches the library's entry point
// through SearchDriver::submitWith, which takes the install function from here.
#include "pssm_query.hpp"

#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <stdexcept>

#include "../../../include/cudasw4_amd_driver.h"
#include "../../../include/cudasw4_amd_pssm.h"
#include "driver_handle.hpp"

namespace swh {

namespace {
const char kColumnLetters[] = "ARNDCQEGHILKMFPSTWYV";

std::vector<std::string> split(const std::string& line) {
    std::vector<std::string> tok;
    std::istringstream ss(line);
    for (std::string t; ss >> t;) tok.push_back(t);
    return tok;
}
bool is_index(const std::string& t) {
    if (t.empty() || t.size() > 9) return false;
    for (char c : t) if (!std::isdigit((unsigned char)c)) return false;
    return true;
}
bool is_integer(const std::string& t) {
    const size_t b = (t[0] == '-' || t[0] == '+') ? 1 : 0;
    if (t.size() == b || t.size() > b + 9) return false;
    for (size_t i = b; i < t.size(); i++) if (!std::isdigit((unsigned char)t[i])) return false;
    return true;
}
bool is_residue(const std::string& t) { return t.size() == 1 && (std::isalpha((unsigned char)t[0]) || t[0] == '*' || t[0] == '-'); }
// 20 (or 20 + 20) single letters: a column header; *ok = it is the expected one
bool is_header(const std::vector<std::string>& tok, bool* ok) {
    if (tok.size() < 20) return false;
    for (const auto& t : tok) if (t.size() != 1 || !std::isalpha((unsigned char)t[0])) return false;
    *ok = tok.size() == 20 || tok.size() == 40;
    for (size_t i = 0; *ok && i < tok.size(); i++) *ok = std::toupper((unsigned char)tok[i][0]) == kColumnLetters[i % 20];
    return true;
}
}  // namespace

PssmQuery read_ascii_pssm(const std::string& path) {
    std::ifstream in(path);
    if (!in) throw std::runtime_error("Cannot open PSSM file " + path);
    auto bad = [&](long line, const std::string& what) { return std::runtime_error(path + ":" + std::to_string(line) + ": " + what); };
    PssmQuery q;
    const size_t slash = path.find_last_of('/');
    q.name = slash == std::string::npos ? path : path.substr(slash + 1);
    bool haveHeader = false;
    long lineno = 0;
    for (std::string line; std::getline(in, line);) {
        lineno++;
        const std::vector<std::string> tok = split(line);
        if (!haveHeader) {
            bool ok = false;
            if (is_header(tok, &ok)) {
                if (!ok) throw bad(lineno, "column header is not 'A R N D C Q E G H I L K M F P S T W Y V'");
                haveHeader = true;
            } else if (tok.size() >= 2 && is_index(tok[0]) && is_residue(tok[1])) {
                throw bad(lineno, "position line before the column header (missing header)");
            }
            continue;
        }
        const bool position = tok.size() >= 2 && is_index(tok[0]) && is_residue(tok[1]);
        if (!position) {
            if (!q.scores.empty()) break;   // blank line / footer behind the positions
            if (tok.empty()) continue;
            throw bad(lineno, "expected a position line (index, residue, 20 scores)");
        }
        const long expect = long(q.length()) + 1;
        if (std::atol(tok[0].c_str()) != expect)
            throw bad(lineno, "position index " + tok[0] + ", expected " + std::to_string(expect) + " (indices must be consecutive from 1)");
        const size_t nvals = tok.size() - 2;
        bool ints = nvals >= 20;
        for (size_t i = 0; ints && i < 20; i++) ints = is_integer(tok[2 + i]);
        if ((nvals != 20 && nvals != 40 && nvals != 42) || !ints)
            throw bad(lineno, "expected 20 integer scores (optionally 20 percentages and 2 information columns), got " + std::to_string(nvals) + " columns");
        for (size_t i = 0; i < 20; i++) {
            const long v = std::atol(tok[2 + i].c_str());
            if (v < -128 || v > 127) throw bad(lineno, "score " + tok[2 + i] + " outside the int8 range");
            q.scores.push_back(int8_t(v));
        }
        q.scores.push_back(kPssmOtherScore);
        q.consensus.push_back(char(std::toupper((unsigned char)tok[1][0])));
    }
    if (!haveHeader) throw bad(lineno > 0 ? lineno : 1, "no column header 'A R N D C Q E G H I L K M F P S T W Y V' found (missing header)");
    if (q.scores.empty()) throw bad(lineno, "no position lines behind the column header");
    return q;
}

void write_ascii_pssm(const std::string& path, const int8_t* pssm, int32_t length, const std::string& consensus) {
    if (!pssm || length <= 0) throw std::runtime_error("empty PSSM");
    if (consensus.size() != size_t(length))
        throw std::runtime_error("consensus has " + std::to_string(consensus.size()) + " residues, the PSSM " + std::to_string(length) + " rows");
    std::ofstream out(path);
    if (!out) throw std::runtime_error("Cannot open file " + path);
    char buf[32];
    out << "\nLast position-specific scoring matrix computed, weighted observed percentages rounded down, "
           "information per position, and relative weight of gapless real matches to pseudocounts\n";
    out << "           ";
    for (int c = 0; c < 20; c++) {
        std::snprintf(buf, sizeof buf, "%5c", kColumnLetters[c]);
        out << buf;
    }
    out << "\n";
    for (int32_t i = 0; i < length; i++) {
        std::snprintf(buf, sizeof buf, "%5d %c  ", int(i + 1), consensus[size_t(i)]);
        out << buf;
        for (int c = 0; c < 20; c++) {
            std::snprintf(buf, sizeof buf, "%5d", int(pssm[size_t(i) * kPssmColumns + c]));
            out << buf;
        }
        out << "\n";
    }
    out.flush();
    if (!out) throw std::runtime_error("Cannot write file " + path);
}

void submit_pssm(SearchDriver& driver, const int8_t* pssm, int32_t length) {
    if (!pssm || length <= 0) throw std::runtime_error("empty PSSM");
    if (length > SW_PSSM_MAX_QUERY_LEN) throw std::runtime_error("PSSM too long");
    for (int32_t i = 0; i < length; i++)
        if (pssm[size_t(i) * kPssmColumns + 20] >= 0)
            throw std::runtime_error("PSSM row " + std::to_string(i) + ": column 20 (other / padding) must be negative");
    driver.submitWith(&sw_set_query_pssm, pssm, size_t(length) * kPssmColumns, length);
}

}  // namespace swh

#ifdef SWH_DRIVER_CAPI   // libcudasw4_host.so (with driver_capi.cpp); `align` links the functions above alone
extern "C" int swdrv_write_pssm_ascii(const char* path, const int8_t* pssm, int32_t qlen, const char* consensus) {
    try {
        if (!path || !consensus) throw std::runtime_error("null path or consensus");
        swh::write_ascii_pssm(path, pssm, qlen, consensus);
        return 0;
    } catch (const std::exception& e) {
        swh::set_driver_error(e.what());
        return -1;
    }
}

extern "C" int swdrv_scan_submit_pssm(swdrv* d, const int8_t* pssm, int32_t qlen) {
    try {
        if (!d || !d->driver) throw std::runtime_error("null driver");
        swh::submit_pssm(*d->driver, pssm, qlen);
        return 0;
    } catch (const std::exception& e) {
        swh::set_driver_error(e.what());
        return -1;
    }
}

extern "C" int swdrv_scan_pssm(swdrv* d, const int8_t* pssm, int32_t qlen, int32_t* scores, int64_t* ids, int cap, int* nres,
                               int* num_overflows, double* seconds, double* gcups) {
    try {
        if (!d || !d->driver) throw std::runtime_error("null driver");
        if (d->driver->inFlight()) throw std::runtime_error("scan() with queries in flight: collect() them first");
    } catch (const std::exception& e) {
        swh::set_driver_error(e.what());
        return -1;
    }
    if (swdrv_scan_submit_pssm(d, pssm, qlen) != 0) return -1;
    return swdrv_scan_collect(d, scores, ids, cap, nres, num_overflows, seconds, gcups);
}
#endif
