// hit_msa.cpp — HitMsa, write_msa, swdrv_hit_msa and swdrv_write_msa: the query-anchored MSA of a query's aligned hits
// (DESIGN.md §17).
//
// Kept out of search_driver.cpp and driver_capi.cpp on purpose (like hit_alignment.cpp and pssm_build.cpp):
// tests/host/fake_gpu links exactly those files against a fake of the C ABI that has no sw_msa_filter.
#include "hit_msa.hpp"

#include <algorithm>
#include <cctype>
#include <fstream>
#include <ostream>
#include <stdexcept>

#include "../../../include/cudasw4_amd_driver.h"
#include "../../../include/cudasw4_amd_msa.h"
#include "../../../include/cudasw4_amd_msa_select.h"
#include "driver_handle.hpp"
#include "sequence_codec.hpp"

namespace swh {

namespace {
void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string("MSA: ") + what + ": " + hipGetErrorString(e));
}
}  // namespace

HitMsa::~HitMsa() {
    if (device_ >= 0 && hipSetDevice(device_) == hipSuccess)
        for (void* b : buf_)
            if (b) (void)hipFree(b);
}

void* HitMsa::grow(int slot, size_t bytes) {
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

MsaFilterResult HitMsa::filter(const char* master, int32_t qlen, const uint8_t* include, int maxIdentity, bool wantRows) {
    if (qlen < 1) throw std::runtime_error("MSA: empty query");
    if (maxIdentity < 0 || maxIdentity > 100) throw std::runtime_error("MSA: the identity threshold must lie in 0 .. 100");
    const HitAligner::Resident res = aligner_.resident();
    if (res.n > size_t(SW_MSA_MAX_HITS)) throw std::runtime_error("MSA: more than " + std::to_string(SW_MSA_MAX_HITS) + " hits");
    if (!res.ctx) throw std::runtime_error("MSA: the hits have not been aligned");
    const size_t n = res.n;
    device_ = res.device;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    sw_msa_args a{};
    if (master) {
        std::vector<int8_t> codes(static_cast<size_t>(qlen));
        for (int32_t i = 0; i < qlen; i++) codes[size_t(i)] = encode_residue(master[i]);
        void* dMaster = grow(kMaster, size_t(qlen));
        hip_check(hipMemcpyAsync(dMaster, codes.data(), size_t(qlen), hipMemcpyHostToDevice, res.stream), "hipMemcpyAsync");
        hip_check(hipStreamSynchronize(res.stream), "hipStreamSynchronize");   // (codes leaves scope)
        a.query = static_cast<const int8_t*>(dMaster);
    }
    a.qlen = qlen;
    a.n = int32_t(n);
    a.chars = res.chars;
    a.offsets = res.offsets;
    a.lengths = res.lengths;
    a.results = res.results;
    a.cigar = res.cigar;
    if (include && n > 0) {
        void* dInclude = grow(kInclude, n);
        hip_check(hipMemcpyAsync(dInclude, include, n, hipMemcpyHostToDevice, res.stream), "hipMemcpyAsync");
        a.include = static_cast<const uint8_t*>(dInclude);
    }
    a.max_identity = maxIdentity;
    const size_t rowBytes = (n + 1) * size_t(qlen);
    if (wantRows) a.rows = static_cast<uint8_t*>(grow(kRows, rowBytes));
    a.residues = static_cast<int32_t*>(grow(kResidues, (n + 1) * sizeof(int32_t)));
    a.keep = static_cast<uint8_t*>(grow(kKeep, n + 1));
    a.purged = static_cast<int32_t*>(grow(kPurged, sizeof(int32_t)));
    a.stream = res.stream;
    size_t need = 0;
    a.temp_bytes_needed = &need;
    if (sw_msa_filter(res.ctx, &a) != SW_OK) throw std::runtime_error(std::string("MSA: sw_msa_filter: ") + sw_last_error());
    a.temp = grow(kTemp, need);
    a.temp_bytes = cap_[kTemp];
    if (sw_msa_filter(res.ctx, &a) != SW_OK) throw std::runtime_error(std::string("MSA: sw_msa_filter: ") + sw_last_error());
    MsaFilterResult out;
    out.keep.resize(n + 1);
    out.residues.resize(n + 1);
    if (wantRows) out.rows.resize(rowBytes);
    hip_check(hipMemcpyAsync(out.keep.data(), a.keep, n + 1, hipMemcpyDeviceToHost, res.stream), "hipMemcpyAsync");
    hip_check(hipMemcpyAsync(out.residues.data(), a.residues, (n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, res.stream), "hipMemcpyAsync");
    hip_check(hipMemcpyAsync(&out.purged, a.purged, sizeof(int32_t), hipMemcpyDeviceToHost, res.stream), "hipMemcpyAsync");
    if (wantRows) hip_check(hipMemcpyAsync(out.rows.data(), a.rows, rowBytes, hipMemcpyDeviceToHost, res.stream), "hipMemcpyAsync");
    hip_check(hipStreamSynchronize(res.stream), "hipStreamSynchronize");
    return out;
}

MsaSelectResult HitMsa::select(const char* master, int32_t qlen, const uint8_t* include, const MsaSelectParams& params, bool wantRows) {
    if (qlen < 1) throw std::runtime_error("MSA: empty query");
    const HitAligner::Resident res = aligner_.resident();
    if (res.n > size_t(SW_MSA_SELECT_MAX_HITS))
        throw std::runtime_error("MSA: the selection takes at most " + std::to_string(SW_MSA_SELECT_MAX_HITS) + " hits");
    if (!res.ctx) throw std::runtime_error("MSA: the hits have not been aligned");
    const size_t n = res.n;
    device_ = res.device;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    sw_msa_select_args a{};
    if (master) {
        std::vector<int8_t> codes(static_cast<size_t>(qlen));
        for (int32_t i = 0; i < qlen; i++) codes[size_t(i)] = encode_residue(master[i]);
        void* dMaster = grow(kMaster, size_t(qlen));
        hip_check(hipMemcpyAsync(dMaster, codes.data(), size_t(qlen), hipMemcpyHostToDevice, res.stream), "hipMemcpyAsync");
        hip_check(hipStreamSynchronize(res.stream), "hipStreamSynchronize");   // (codes leaves scope)
        a.query = static_cast<const int8_t*>(dMaster);
    }
    a.qlen = qlen;
    a.n = int32_t(n);
    a.chars = res.chars;
    a.offsets = res.offsets;
    a.lengths = res.lengths;
    a.results = res.results;
    a.cigar = res.cigar;
    if (include && n > 0) {
        void* dInclude = grow(kInclude, n);
        hip_check(hipMemcpyAsync(dInclude, include, n, hipMemcpyHostToDevice, res.stream), "hipMemcpyAsync");
        a.include = static_cast<const uint8_t*>(dInclude);
    }
    a.min_coverage = params.minCoverage;
    a.min_query_identity = params.minQueryIdentity;
    a.diff = params.diff;
    a.ladder = params.ladder.data();
    a.n_ladder = int32_t(params.ladder.size());
    const size_t rowBytes = (n + 1) * size_t(qlen);
    if (wantRows) a.rows = static_cast<uint8_t*>(grow(kRows, rowBytes));
    a.residues = static_cast<int32_t*>(grow(kResidues, (n + 1) * sizeof(int32_t)));
    a.state = static_cast<uint8_t*>(grow(kState, n + 1));
    a.counts = static_cast<int32_t*>(grow(kCounts, 4 * sizeof(int32_t)));
    a.depth = static_cast<int32_t*>(grow(kDepth, size_t(qlen) * sizeof(int32_t)));
    a.stream = res.stream;
    size_t need = 0;
    a.temp_bytes_needed = &need;
    if (sw_msa_select(res.ctx, &a) != SW_OK) throw std::runtime_error(std::string("MSA: sw_msa_select: ") + sw_last_error());
    a.temp = grow(kTemp, need);
    a.temp_bytes = cap_[kTemp];
    if (sw_msa_select(res.ctx, &a) != SW_OK) throw std::runtime_error(std::string("MSA: sw_msa_select: ") + sw_last_error());
    MsaSelectResult out;
    out.state.resize(n + 1);
    out.residues.resize(n + 1);
    out.depth.resize(size_t(qlen));
    if (wantRows) out.rows.resize(rowBytes);
    hip_check(hipMemcpyAsync(out.state.data(), a.state, n + 1, hipMemcpyDeviceToHost, res.stream), "hipMemcpyAsync");
    hip_check(hipMemcpyAsync(out.residues.data(), a.residues, (n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, res.stream), "hipMemcpyAsync");
    hip_check(hipMemcpyAsync(out.counts, a.counts, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, res.stream), "hipMemcpyAsync");
    hip_check(hipMemcpyAsync(out.depth.data(), a.depth, size_t(qlen) * sizeof(int32_t), hipMemcpyDeviceToHost, res.stream), "hipMemcpyAsync");
    if (wantRows) hip_check(hipMemcpyAsync(out.rows.data(), a.rows, rowBytes, hipMemcpyDeviceToHost, res.stream), "hipMemcpyAsync");
    hip_check(hipStreamSynchronize(res.stream), "hipStreamSynchronize");
    return out;
}

bool parse_msa_format(const std::string& name, MsaFormat& out) {
    if (name == "a3m") out = MsaFormat::A3m;
    else if (name == "fasta") out = MsaFormat::Fasta;
    else return false;
    return true;
}

std::string msa_line(MsaFormat format, int32_t qlen, const std::string& s, const HitAlignment& a) {
    std::string line;
    line.reserve(size_t(qlen) + 16);
    int64_t columns = std::max<int32_t>(a.r.q_begin, 0);   // upper-case letters and '-' so far
    line.append(size_t(columns), '-');
    int64_t j = a.r.s_begin;
    // (a DB decodes its "other" code as '-', which an alignment line cannot carry as a residue: 'X')
    auto letter = [&](int64_t at) {
        const char c = at >= 0 && at < int64_t(s.size()) ? s[size_t(at)] : 'X';
        return std::isalpha((unsigned char)c) ? c : 'X';
    };
    for (const uint32_t w : a.cigar) {
        const int64_t len = int64_t(w >> 4);
        const uint32_t op = w & 15u;
        if (op == SW_CIGAR_EQ || op == SW_CIGAR_X) {
            for (int64_t k = 0; k < len; k++) line.push_back(char(std::toupper((unsigned char)letter(j + k))));
            j += len;
            columns += len;
        } else if (op == SW_CIGAR_I) {
            line.append(size_t(len), '-');
            columns += len;
        } else if (op == SW_CIGAR_D) {
            if (format == MsaFormat::A3m)
                for (int64_t k = 0; k < len; k++) line.push_back(char(std::tolower((unsigned char)letter(j + k))));
            j += len;
        }
    }
    if (columns > qlen) throw std::runtime_error("MSA: an alignment has more query columns than the query has residues");
    line.append(size_t(qlen - columns), '-');
    return line;
}

size_t write_msa(std::ostream& os, MsaFormat format, const std::string& master, const std::string& queryHeader,
                 const std::vector<std::string>& headers, const std::vector<std::string>& subjectLetters,
                 const std::vector<HitAlignment>& alignments, const uint8_t* keep) {
    if (headers.size() != alignments.size() || subjectLetters.size() != alignments.size())
        throw std::runtime_error("MSA: headers, subjects and alignments differ in number");
    os << '>' << queryHeader << '\n' << master << '\n';
    size_t written = 0;
    for (size_t h = 0; h < alignments.size(); h++) {
        const HitAlignment& a = alignments[h];
        if ((keep && !keep[h]) || a.r.status != SW_ALIGN_OK || a.cigar.empty()) continue;
        os << '>' << headers[h] << '\n' << msa_line(format, int32_t(master.size()), subjectLetters[h], a) << '\n';
        written++;
    }
    return written;
}

size_t write_msa(const std::string& path, MsaFormat format, const std::string& master, const std::string& queryHeader,
                 const std::vector<std::string>& headers, const std::vector<std::string>& subjectLetters,
                 const std::vector<HitAlignment>& alignments, const uint8_t* keep) {
    std::ofstream os(path);
    if (!os) throw std::runtime_error("MSA: cannot open " + path + " for writing");
    const size_t written = write_msa(os, format, master, queryHeader, headers, subjectLetters, alignments, keep);
    os.flush();
    if (!os) throw std::runtime_error("MSA: writing " + path + " failed");
    return written;
}

}  // namespace swh

#ifdef SWH_DRIVER_CAPI   // libcudasw4_host.so (with driver_capi.cpp); `align` links the functions above alone
extern "C" int swdrv_write_msa(const char* path, int format, const char* master_letters, const char* query_header, int n,
                               const char* const* headers, const char* const* subject_letters, const sw_align_result* results,
                               const uint32_t* cigar, const uint8_t* keep) {
    try {
        if (!path || !master_letters || !query_header || n < 0 || (n > 0 && (!headers || !subject_letters || !results || !cigar)))
            throw std::runtime_error("MSA: bad arguments");
        if (format != 0 && format != 1) throw std::runtime_error("MSA: format must be 0 (a3m) or 1 (fasta)");
        const size_t count = static_cast<size_t>(n);
        std::vector<std::string> hs(count), ss(count);
        std::vector<swh::HitAlignment> al(count);
        for (int h = 0; h < n; h++) {
            hs[size_t(h)] = headers[h];
            ss[size_t(h)] = subject_letters[h];
            al[size_t(h)].r = results[h];
            if (results[h].cigar_len > 0)
                al[size_t(h)].cigar.assign(cigar + results[h].cigar_offset, cigar + results[h].cigar_offset + results[h].cigar_len);
        }
        swh::write_msa(std::string(path), format == 0 ? swh::MsaFormat::A3m : swh::MsaFormat::Fasta, master_letters, query_header, hs, ss,
                       al, keep);
        return 0;
    } catch (const std::exception& e) {
        swh::set_driver_error(e.what());
        return -1;
    }
}

extern "C" int swdrv_hit_msa(swdrv* d, const char* master_letters, int32_t qlen, const int8_t* pssm, const int64_t* ids,
                             const int32_t* scores, int n, int max_identity, const char* query_header, const char* out_path,
                             int format, sw_align_result* results, uint32_t* cigar, int64_t cigar_cap, uint8_t* rows,
                             int32_t* residues, uint8_t* keep, int32_t* purged) {
    try {
        if (!d || !d->driver) throw std::runtime_error("null driver");
        if (!master_letters || qlen < 1 || n < 0 || (n > 0 && (!ids || !scores))) throw std::runtime_error("MSA: bad arguments");
        if (format != 0 && format != 1) throw std::runtime_error("MSA: format must be 0 (a3m) or 1 (fasta)");
        swh::HitAligner aligner(*d->driver);
        const std::vector<swh::HitAlignment> hits = pssm ? aligner.align(pssm, qlen, master_letters, ids, scores, size_t(n))
                                                         : aligner.align(master_letters, qlen, ids, scores, size_t(n));
        swh::HitMsa msa(aligner);
        swh::MsaFilterResult f;
        if (n > 0) f = msa.filter(master_letters, qlen, nullptr, max_identity, rows != nullptr);
        else {   // (no align() call behind an empty list: the master alone)
            f.keep.assign(1, 0);
            f.residues.assign(1, 0);
            for (int32_t i = 0; i < qlen; i++) f.residues[0] += swh::encode_residue(master_letters[i]) < 20;
            f.keep[0] = f.residues[0] > 0;
            if (rows)
                for (int32_t i = 0; i < qlen; i++) rows[i] = uint8_t(std::min<int>(swh::encode_residue(master_letters[i]), 20));
        }
        int64_t used = 0;
        for (size_t i = 0; i < hits.size(); i++) {
            if (results) {
                results[i] = hits[i].r;
                results[i].cigar_offset = used;
            }
            if (cigar) {
                if (used + int64_t(hits[i].cigar.size()) > cigar_cap) throw std::runtime_error("cigar_cap too small");
                std::copy(hits[i].cigar.begin(), hits[i].cigar.end(), cigar + used);
            }
            used += int64_t(hits[i].cigar.size());
        }
        if (rows && n > 0) std::copy(f.rows.begin(), f.rows.end(), rows);
        if (residues) std::copy(f.residues.begin(), f.residues.end(), residues);
        if (keep) std::copy(f.keep.begin(), f.keep.end(), keep);
        if (purged) *purged = f.purged;
        if (out_path) {
            const size_t count = static_cast<size_t>(n);
        std::vector<std::string> hs(count), ss(count);
            for (int h = 0; h < n; h++) {
                hs[size_t(h)] = std::string(d->driver->getReferenceHeader(ids[h]));
                ss[size_t(h)] = d->driver->getReferenceSequence(ids[h]);
            }
            swh::write_msa(std::string(out_path), format == 0 ? swh::MsaFormat::A3m : swh::MsaFormat::Fasta,
                           std::string(master_letters, size_t(qlen)), query_header ? query_header : "query", hs, ss, hits, f.keep.data());
        }
        return 0;
    } catch (const std::exception& e) {
        swh::set_driver_error(e.what());
        return -1;
    }
}

extern "C" int swdrv_hit_msa_select(swdrv* d, const char* master_letters, int32_t qlen, const int8_t* pssm, const int64_t* ids,
                                    const int32_t* scores, int n, int min_coverage, int min_query_identity, int diff,
                                    const int32_t* ladder, int n_ladder, const char* query_header, const char* out_path, int format,
                                    sw_align_result* results, uint32_t* cigar, int64_t cigar_cap, uint8_t* rows, int32_t* residues,
                                    uint8_t* state, int32_t* depth, int32_t* counts) {
    try {
        if (!d || !d->driver) throw std::runtime_error("null driver");
        if (!master_letters || qlen < 1 || n < 0 || (n > 0 && (!ids || !scores))) throw std::runtime_error("MSA: bad arguments");
        if (format != 0 && format != 1) throw std::runtime_error("MSA: format must be 0 (a3m) or 1 (fasta)");
        if (!ladder || n_ladder < 1 || n_ladder > SW_MSA_SELECT_MAX_LADDER) throw std::runtime_error("MSA: the ladder needs 1 .. 16 rungs");
        swh::MsaSelectParams params;
        params.minCoverage = min_coverage;
        params.minQueryIdentity = min_query_identity;
        params.diff = diff;
        params.ladder.assign(ladder, ladder + n_ladder);
        swh::HitAligner aligner(*d->driver);
        std::vector<swh::HitAlignment> hits;
        if (n > 0)
            hits = pssm ? aligner.align(pssm, qlen, master_letters, ids, scores, size_t(n)) : aligner.align(master_letters, qlen, ids, scores, size_t(n));
        swh::MsaSelectResult f;
        if (n > 0) {
            swh::HitMsa msa(aligner);
            f = msa.select(master_letters, qlen, nullptr, params, rows != nullptr);
        } else {   // (no align() call behind an empty list: the master alone)
            f.state.assign(1, 0);
            f.residues.assign(1, 0);
            f.depth.assign(size_t(qlen), 0);
            for (int32_t i = 0; i < qlen; i++) f.depth[size_t(i)] = swh::encode_residue(master_letters[i]) < 20;
            for (int32_t i = 0; i < qlen; i++) f.residues[0] += f.depth[size_t(i)];
            f.state[0] = f.residues[0] > 0;
            if (!f.state[0]) f.depth.assign(size_t(qlen), 0);
            if (rows)
                for (int32_t i = 0; i < qlen; i++) rows[i] = uint8_t(std::min<int>(swh::encode_residue(master_letters[i]), 20));
        }
        int64_t used = 0;
        for (size_t i = 0; i < hits.size(); i++) {
            if (results) {
                results[i] = hits[i].r;
                results[i].cigar_offset = used;
            }
            if (cigar) {
                if (used + int64_t(hits[i].cigar.size()) > cigar_cap) throw std::runtime_error("cigar_cap too small");
                std::copy(hits[i].cigar.begin(), hits[i].cigar.end(), cigar + used);
            }
            used += int64_t(hits[i].cigar.size());
        }
        if (rows && n > 0) std::copy(f.rows.begin(), f.rows.end(), rows);
        if (residues) std::copy(f.residues.begin(), f.residues.end(), residues);
        if (state) std::copy(f.state.begin(), f.state.end(), state);
        if (depth) std::copy(f.depth.begin(), f.depth.end(), depth);
        if (counts) std::copy(f.counts, f.counts + 4, counts);
        if (out_path) {
            const size_t count = static_cast<size_t>(n);
            std::vector<std::string> hs(count), ss(count);
            std::vector<uint8_t> keep(count + 1, 0);
            for (int h = 0; h < n; h++) {
                hs[size_t(h)] = std::string(d->driver->getReferenceHeader(ids[h]));
                ss[size_t(h)] = d->driver->getReferenceSequence(ids[h]);
                keep[size_t(h)] = f.state[size_t(h)] == SW_MSA_STATE_KEPT;
            }
            swh::write_msa(std::string(out_path), format == 0 ? swh::MsaFormat::A3m : swh::MsaFormat::Fasta,
                           std::string(master_letters, size_t(qlen)), query_header ? query_header : "query", hs, ss, hits, keep.data());
        }
        return 0;
    } catch (const std::exception& e) {
        swh::set_driver_error(e.what());
        return -1;
    }
}
#endif
