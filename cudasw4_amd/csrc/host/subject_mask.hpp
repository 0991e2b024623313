// subject_mask.hpp — low-complexity masking of subjects, host side (include/cudasw4_amd_mask.h): the bits-to-sums
// conversion and the scalar statement of the rule the device kernels implement (sw_mask_subjects).  The driver masks the
// database on the device; the few hundred subjects that hit alignment and the shuffled calibration gather from the host copy
// of the DB go through mask_subject here, and sw_align_hits' score check holds the two statements against each other.
#pragma once
#include <cstdint>

namespace swh {

constexpr int kMaskDefaultWindow = 12;
constexpr double kMaskDefaultTriggerBits = 1.9, kMaskDefaultExtendBits = 2.2;

struct MaskParams {   // sw_mask_params
    int32_t window = kMaskDefaultWindow;
    int32_t triggerSum = 20705;   // mask_threshold(12, 1.9)
    int32_t extendSum = 17019;    // mask_threshold(12, 2.2)
};

// max(1, ceil(1024 W (log2 W - bits))): the sum a window of W letters reaches at `bits` of Shannon entropy
int32_t mask_threshold(int window, double bits);
// window 4 .. 32, 1 <= extendSum <= triggerSum; throws std::runtime_error otherwise
void check_mask_params(const MaskParams& p);
// the parameters of (window, trigger bits, extend bits), checked: trigger <= extend in bits
MaskParams mask_params_from_bits(int window, double triggerBits, double extendBits);

// out[0 .. L) = codes[0 .. L) with the positions of masked segments replaced by code 20; out may be codes.  Returns the number
// of positions the segments cover.
int64_t mask_subject(const int8_t* codes, int32_t L, const MaskParams& p, int8_t* out);

class SearchDriver;
// SearchDriver::setSubjectMasking with the device function of this translation unit (sw_mask_subjects, in place); nullptr: off
void enable_subject_masking(SearchDriver& driver, const MaskParams* params);

}  // namespace swh
