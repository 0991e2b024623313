// pssm_build.cpp — pssm_from_counts, PssmBuilder, swdrv_pssm_from_counts and swdrv_build_pssm: a PSSM from a query's aligned
// hits (DESIGN.md "Building a PSSM").
//
// Kept out of search_driver.cpp and driver_capi.cpp on purpose (like hit_alignment.cpp and pssm_query.cpp):
// tests/host/fake_gpu links exactly those files against a fake of the C ABI that has no sw_pssm_accumulate.
#include "pssm_build.hpp"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

#include "../../../include/cudasw4_amd_driver.h"
#include "../../../include/cudasw4_amd_pssm.h"
#include "driver_handle.hpp"

namespace swh {

namespace {

constexpr int kStd = 20;   // standard residues
// Robinson & Robinson (1991) background frequencies in per mille, code order ARNDCQEGHILKMFPSTWYV; they sum to 1000
const double kBackground[kStd] = {78.05, 51.29, 44.87, 53.64, 19.25, 42.64, 62.95, 73.77, 21.99, 51.42,
                                  90.19, 57.44, 22.43, 38.56, 52.03, 71.20, 58.41, 13.30, 32.16, 64.41};

void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string("PSSM build: ") + what + ": " + hipGetErrorString(e));
}

}  // namespace

const SubstitutionMatrix& pssm_table_of(MatrixId id) { return substitution_matrix(MatrixId(int(id) % 4)); }

double pssm_lambda(const SubstitutionMatrix& t) {
    if (t.dim != 21) throw std::runtime_error("PSSM build: lambda is defined on the 21-letter tables");
    auto f = [&](double lambda) {
        double sum = 0;
        for (int a = 0; a < kStd; a++)
            for (int b = 0; b < kStd; b++)
                sum += kBackground[a] * 1e-3 * kBackground[b] * 1e-3 * std::exp(lambda * t.m[size_t(a * 21 + b)]);
        return sum - 1.0;
    };
    double lo = 1e-3, hi = 2.0;
    if (!(f(lo) < 0 && f(hi) > 0)) throw std::runtime_error("PSSM build: the table has no lambda in [0.001, 2]");
    for (;;) {
        const double mid = 0.5 * (lo + hi);
        if (mid <= lo || mid >= hi) break;
        if (f(mid) > 0) hi = mid;
        else lo = mid;
    }
    return lo;
}

void pssm_from_counts(const SubstitutionMatrix& t, const int8_t* master, int32_t qlen, const uint32_t* counts,
                      const uint64_t* wcounts, double beta, int8_t* out, double* raw, double* lambdaOut) {
    if (t.dim != 21) throw std::runtime_error("PSSM build: the conversion takes a 21-letter table");
    if (qlen < 1 || !master || !counts || !wcounts || !out) throw std::runtime_error("PSSM build: empty query or null buffer");
    if (!(beta > 0) || !std::isfinite(beta)) throw std::runtime_error("PSSM build: the pseudocount must be positive");
    for (int r = 0; r < 21; r++)
        if (t.m[size_t(r * 21 + 20)] >= 0)
            throw std::runtime_error("PSSM build: column 20 (other / padding) of the table must be negative");
    const double lambda = pssm_lambda(t);
    if (lambdaOut) *lambdaOut = lambda;
    double p[kStd], e[kStd][kStd];   // e[a][b] = q_ab / p_b = p_a exp(lambda s_ab)
    for (int a = 0; a < kStd; a++) p[a] = kBackground[a] * 1e-3;
    for (int a = 0; a < kStd; a++)
        for (int b = 0; b < kStd; b++) e[a][b] = p[a] * std::exp(lambda * t.m[size_t(a * 21 + b)]);
    for (int32_t i = 0; i < qlen; i++) {
        const int m = master[i] >= 0 && master[i] < 20 ? master[i] : 20;
        int8_t* row = out + size_t(i) * 21;
        double* rrow = raw ? raw + size_t(i) * kStd : nullptr;
        const uint32_t* c = counts + size_t(i) * kStd;
        const uint64_t* w = wcounts + size_t(i) * kStd;
        row[20] = t.m[size_t(m * 21 + 20)];
        uint64_t total = 0;
        int k = 0;
        for (int a = 0; a < kStd; a++) {
            total += w[a];
            k += c[a] > 0;
        }
        if (total == 0) {
            for (int a = 0; a < kStd; a++) {
                row[a] = t.m[size_t(m * 21 + a)];
                if (rrow) rrow[a] = row[a];
            }
            continue;
        }
        double f[kStd];
        for (int a = 0; a < kStd; a++) f[a] = double(w[a]) / double(total);
        const double alpha = k - 1;
        for (int a = 0; a < kStd; a++) {
            double g = 0;
            for (int b = 0; b < kStd; b++) g += f[b] * e[a][b];
            const double q = (alpha * f[a] + beta * g) / (alpha + beta);
            const double r = std::log(q / p[a]) / lambda;
            if (rrow) rrow[a] = r;
            row[a] = int8_t(std::min(127.0, std::max(-128.0, std::round(r))));   // (round: halves away from zero)
        }
    }
}

PssmBuilder::~PssmBuilder() {
    if (device_ >= 0 && hipSetDevice(device_) == hipSuccess)
        for (void* b : buf_)
            if (b) (void)hipFree(b);
}

void* PssmBuilder::grow(int slot, size_t bytes) {
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

std::vector<int8_t> PssmBuilder::build(const char* master, int32_t qlen, const int8_t* pssm, const int64_t* ids,
                                       const int32_t* scores, size_t n, int32_t minScore, double pseudocount, PssmBuildInfo* info,
                                       const uint8_t* admitted, int maxHsps, int hspMinScore, int purgeIdentity) {
    if (qlen < 1 || !master) throw std::runtime_error("PSSM build: empty master sequence");
    if (qlen > (1 << 20)) throw std::runtime_error("PSSM build: queries longer than 2^20 residues are not supported");
    if (n > 0 && (!ids || !scores)) throw std::runtime_error("PSSM build: null hit list");
    if (!(pseudocount > 0)) throw std::runtime_error("PSSM build: the pseudocount must be positive");
    if (purgeIdentity < 0 || purgeIdentity > 100) throw std::runtime_error("PSSM build: the purge identity must lie in 0 .. 100");
    PssmBuildInfo local;
    PssmBuildInfo& I = info ? *info : local;
    I = PssmBuildInfo();
    if (maxHsps > 1) {
        I.hsps = pssm ? aligner_.align(pssm, qlen, master, ids, scores, n, maxHsps, hspMinScore)
                      : aligner_.align(master, qlen, ids, scores, n, maxHsps, hspMinScore);
        I.alignments.resize(n);
        for (size_t h = 0; h < n; h++) I.alignments[h] = I.hsps[h].front();
    } else {
        I.alignments = pssm ? aligner_.align(pssm, qlen, master, ids, scores, n) : aligner_.align(master, qlen, ids, scores, n);
    }
    const HitAligner::Resident res = aligner_.resident();
    if (res.n != n) throw std::runtime_error("PSSM build: internal error (resident hits)");
    // the inclusion rule
    I.included.assign(n, 0);
    int32_t expectUsed = 0;
    for (size_t h = 0; h < n; h++) {
        const sw_align_result& r = I.alignments[h].r;
        if (admitted ? !admitted[h] : scores[h] < minScore) I.belowScore++;
        else if (r.status == SW_ALIGN_NO_TRACE) I.noTrace++;
        else if (r.status == SW_ALIGN_OK && r.q_begin == 0 && r.q_end == qlen && r.identities == qlen && r.columns == qlen) I.copies++;
        else if (r.status == SW_ALIGN_OK && r.cigar_len > 0) {
            I.included[h] = 1;
            expectUsed++;
        }
    }
    if (purgeIdentity > 0 && n > 0) {
        // the redundancy filter on the hits that passed, with their include bytes: include[h] &= keep[h]
        if (!msa_) msa_ = std::make_unique<HitMsa>(aligner_);
        const MsaFilterResult f = msa_->filter(master, qlen, I.included.data(), purgeIdentity, false);
        I.purged = f.purged;
        for (size_t h = 0; h < n; h++)
            if (I.included[h] && !f.keep[h]) {
                I.included[h] = 0;
                expectUsed--;
            }
    }
    std::vector<int8_t> codes(static_cast<size_t>(qlen));
    for (int32_t i = 0; i < qlen; i++) codes[size_t(i)] = encode_residue(master[i]);

    device_ = res.device;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    const size_t cells = size_t(qlen) * kStd;
    sw_pssm_accumulate_args a{};
    void* dMaster = grow(kMaster, size_t(qlen));
    hip_check(hipMemcpyAsync(dMaster, codes.data(), size_t(qlen), hipMemcpyHostToDevice, res.stream), "hipMemcpyAsync");
    a.query = static_cast<const int8_t*>(dMaster);
    a.qlen = qlen;
    a.n = int32_t(n);
    a.chars = res.chars;
    a.offsets = res.offsets;
    a.lengths = res.lengths;
    a.results = res.results;
    a.cigar = res.cigar;
    if (n > 0) {
        void* dInclude = grow(kInclude, n);
        hip_check(hipMemcpyAsync(dInclude, I.included.data(), n, hipMemcpyHostToDevice, res.stream), "hipMemcpyAsync");
        a.include = static_cast<const uint8_t*>(dInclude);
    }
    a.counts = static_cast<uint32_t*>(grow(kCounts, cells * sizeof(uint32_t)));
    a.weights = static_cast<uint64_t*>(grow(kWeights, (n + 1) * sizeof(uint64_t)));
    a.wcounts = static_cast<uint64_t*>(grow(kWcounts, cells * sizeof(uint64_t)));
    a.used = static_cast<int32_t*>(grow(kUsed, sizeof(int32_t)));
    a.stream = res.stream;
    if (sw_pssm_accumulate(res.ctx, &a) != SW_OK) throw std::runtime_error(std::string("PSSM build: sw_pssm_accumulate: ") + sw_last_error());
    std::vector<uint32_t> counts(cells);
    std::vector<uint64_t> wcounts(cells);
    int32_t used = -1;
    hip_check(hipMemcpyAsync(counts.data(), a.counts, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, res.stream), "hipMemcpyAsync");
    hip_check(hipMemcpyAsync(wcounts.data(), a.wcounts, cells * sizeof(uint64_t), hipMemcpyDeviceToHost, res.stream), "hipMemcpyAsync");
    hip_check(hipMemcpyAsync(&used, a.used, sizeof(int32_t), hipMemcpyDeviceToHost, res.stream), "hipMemcpyAsync");
    hip_check(hipStreamSynchronize(res.stream), "hipStreamSynchronize");
    if (used != expectUsed) throw std::runtime_error("PSSM build: internal error (the device counted " + std::to_string(used) +
                                                     " participating hits, the host " + std::to_string(expectUsed) + ")");
    I.used = used;
    std::vector<int8_t> out(size_t(qlen) * 21);
    pssm_from_counts(pssm_table_of(d_.matrix().id), codes.data(), qlen, counts.data(), wcounts.data(), pseudocount, out.data(),
                     nullptr, &I.lambda);
    return out;
}

}  // namespace swh

#ifdef SWH_DRIVER_CAPI   // libcudasw4_host.so (with driver_capi.cpp); `align` links the functions above alone
namespace {
int build_pssm_capi(swdrv* d, const char* master_letters, int32_t qlen, const int8_t* pssm, const int64_t* ids, const int32_t* scores,
                    int n, int32_t min_score, double pseudocount, int purge_identity, int8_t* pssm_out, swdrv_pssm_info* info_out,
                    int32_t* purged_out) {
    try {
        if (!d || !d->driver) throw std::runtime_error("null driver");
        if (n < 0 || !pssm_out) throw std::runtime_error("bad arguments");
        swh::HitAligner aligner(*d->driver);
        swh::PssmBuilder builder(*d->driver, aligner);
        swh::PssmBuildInfo info;
        const std::vector<int8_t> out = builder.build(master_letters, qlen, pssm, ids, scores, size_t(n), min_score, pseudocount, &info,
                                                      nullptr, 1, 1, purge_identity);
        std::copy(out.begin(), out.end(), pssm_out);
        if (info_out) {
            info_out->used = info.used;
            info_out->below_score = info.belowScore;
            info_out->no_trace = info.noTrace;
            info_out->copies = info.copies;
            info_out->lambda = info.lambda;
            if (info_out->included) std::copy(info.included.begin(), info.included.end(), info_out->included);
        }
        if (purged_out) *purged_out = info.purged;
        return 0;
    } catch (const std::exception& e) {
        swh::set_driver_error(e.what());
        return -1;
    }
}
}  // namespace

extern "C" int swdrv_pssm_from_counts(int matrix, const int8_t* master_codes, int32_t qlen, const uint32_t* counts,
                                      const uint64_t* wcounts, double pseudocount, int8_t* pssm_out, double* raw_out,
                                      double* lambda_out) {
    try {
        swh::MatrixId id;
        const int base = matrix > 100 ? matrix / 100 : matrix;
        if ((matrix > 100 && matrix % 100 != 25) || !swh::parse_matrix_name("blosum" + std::to_string(base), id))
            throw std::runtime_error("unknown matrix");
        swh::pssm_from_counts(swh::pssm_table_of(id), master_codes, qlen, counts, wcounts, pseudocount, pssm_out, raw_out, lambda_out);
        return 0;
    } catch (const std::exception& e) {
        swh::set_driver_error(e.what());
        return -1;
    }
}

extern "C" int swdrv_build_pssm(swdrv* d, const char* master_letters, int32_t qlen, const int8_t* pssm, const int64_t* ids,
                                const int32_t* scores, int n, int32_t min_score, double pseudocount, int8_t* pssm_out,
                                swdrv_pssm_info* info_out) {
    return build_pssm_capi(d, master_letters, qlen, pssm, ids, scores, n, min_score, pseudocount, 0, pssm_out, info_out, nullptr);
}

extern "C" int swdrv_build_pssm_purged(swdrv* d, const char* master_letters, int32_t qlen, const int8_t* pssm, const int64_t* ids,
                                       const int32_t* scores, int n, int32_t min_score, double pseudocount, int purge_identity,
                                       int8_t* pssm_out, swdrv_pssm_info* info_out, int32_t* purged_out) {
    return build_pssm_capi(d, master_letters, qlen, pssm, ids, scores, n, min_score, pseudocount, purge_identity, pssm_out, info_out,
                           purged_out);
}
#endif
