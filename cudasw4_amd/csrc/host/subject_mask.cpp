// subject_mask.cpp — see subject_mask.hpp.  Also the C ABI that needs no GPU, swdrv_mask_threshold / swdrv_mask_subject, and
// the driver's: swdrv_set_subject_masking / swdrv_masking_counts.
#include "subject_mask.hpp"

#include <cmath>
#include <stdexcept>
#include <vector>

#include "../../../include/cudasw4_amd_mask.h"
#include "driver_handle.hpp"

namespace swh {

int32_t mask_threshold(int window, double bits) {
    const double v = std::ceil(1024.0 * double(window) * (std::log2(double(window)) - bits));
    return v < 1.0 ? 1 : int32_t(v);
}

void check_mask_params(const MaskParams& p) {
    if (p.window < SW_MASK_MIN_WINDOW || p.window > SW_MASK_MAX_WINDOW) throw std::runtime_error("subject masking: the window must be 4 .. 32");
    if (p.extendSum < 1 || p.triggerSum < p.extendSum) throw std::runtime_error("subject masking: 1 <= extend sum <= trigger sum is required");
}

MaskParams mask_params_from_bits(int window, double triggerBits, double extendBits) {
    if (window < SW_MASK_MIN_WINDOW || window > SW_MASK_MAX_WINDOW) throw std::runtime_error("subject masking: the window must be 4 .. 32");
    if (!(triggerBits <= extendBits)) throw std::runtime_error("subject masking: the trigger entropy must not be above the extension entropy");
    MaskParams p;
    p.window = window;
    p.triggerSum = mask_threshold(window, triggerBits);
    p.extendSum = mask_threshold(window, extendBits);
    check_mask_params(p);
    return p;
}

int64_t mask_subject(const int8_t* codes, int32_t L, const MaskParams& p, int8_t* out) {
    static const int32_t U[SW_MASK_MAX_WINDOW + 1] = {SW_MASK_U_TABLE};
    check_mask_params(p);
    const int32_t W = p.window;
    std::vector<char> masked(size_t(L > 0 ? L : 0), 0);
    int32_t count[20] = {0};
    int32_t S = 0;   // of the window [i, i + W): kept up as a letter leaves and one enters
    auto move = [&](int8_t code, int32_t by) {
        const unsigned c = uint8_t(code);
        if (c >= 20) return;   // a letter of its own
        S -= count[c] * U[count[c]];
        count[c] += by;
        S += count[c] * U[count[c]];
    };
    for (int32_t k = 0; k < W - 1 && k < L; k++) move(codes[k], +1);
    int32_t runStart = -1;
    bool triggered = false;
    for (int32_t i = 0; i + W <= L + 1; i++) {   // i == L - W + 1: behind the last window, closes an open run
        bool lo = false;
        if (i + W <= L) {
            move(codes[i + W - 1], +1);
            lo = S >= p.extendSum;
            if (lo && runStart < 0) { runStart = i; triggered = false; }
            if (lo && S >= p.triggerSum) triggered = true;
            move(codes[i], -1);
        }
        if (!lo && runStart >= 0) {
            if (triggered)
                for (int32_t k = runStart; k < i - 1 + W; k++) masked[size_t(k)] = 1;
            runStart = -1;
        }
    }
    int64_t covered = 0;
    for (int32_t k = 0; k < L; k++) {
        out[k] = masked[size_t(k)] ? int8_t(SW_MASK_CODE) : codes[k];
        covered += masked[size_t(k)];
    }
    return covered;
}

}  // namespace swh

namespace {
// SearchDriver::SubjectMaskFn: sw_mask_subjects in place
int mask_on_device(sw_ctx* ctx, int8_t* chars, const uint64_t* offsets, const int32_t* lengths, int32_t n, const swh::MaskParams& params,
                   void* temp, size_t tempBytes, size_t* tempBytesNeeded, unsigned long long* counts, void* stream) {
    const sw_mask_params p{params.window, params.triggerSum, params.extendSum};
    return sw_mask_subjects(ctx, chars, offsets, lengths, n, &p, chars, temp, tempBytes, tempBytesNeeded, counts, stream);
}
}  // namespace

namespace swh {
void enable_subject_masking(SearchDriver& driver, const MaskParams* params) {
    if (params) driver.setSubjectMasking(&mask_on_device, *params);
    else driver.setSubjectMasking(nullptr, MaskParams());
}
}  // namespace swh

#ifdef SWH_DRIVER_CAPI   // libcudasw4_host.so (with driver_capi.cpp); `align` links the functions above alone
extern "C" int32_t swdrv_mask_threshold(int32_t window, double bits) { return swh::mask_threshold(window, bits); }

// -1: parameters out of range
extern "C" int64_t swdrv_mask_subject(const int8_t* codes, int32_t length, int32_t window, int32_t trigger_sum, int32_t extend_sum,
                                      int8_t* out) {
    try {
        swh::MaskParams p;
        p.window = window; p.triggerSum = trigger_sum; p.extendSum = extend_sum;
        return swh::mask_subject(codes, length, p, out);
    } catch (const std::exception&) {
        return -1;
    }
}

extern "C" int swdrv_set_subject_masking(swdrv* d, int on, int32_t window, double trigger_bits, double extend_bits) {
    try {
        if (!d) throw std::runtime_error("null driver");
        if (on) {
            const swh::MaskParams p = swh::mask_params_from_bits(window, trigger_bits, extend_bits);
            swh::enable_subject_masking(*d->driver, &p);
        } else {
            swh::enable_subject_masking(*d->driver, nullptr);
        }
        return 0;
    } catch (const std::exception& e) {
        swh::set_driver_error(e.what());
        return -1;
    }
}

extern "C" int swdrv_masking_counts(swdrv* d, uint64_t* positions, uint64_t* subjects, uint64_t* residues_seen) {
    try {
        if (!d) throw std::runtime_error("null driver");
        const swh::SearchDriver::MaskingCounts c = d->driver->maskingCounts();
        if (positions) *positions = c.positions;
        if (subjects) *subjects = c.subjects;
        if (residues_seen) *residues_seen = c.residuesSeen;
        return 0;
    } catch (const std::exception& e) {
        swh::set_driver_error(e.what());
        return -1;
    }
}
#endif
