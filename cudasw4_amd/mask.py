"""Low-complexity masking of subjects: the rule of include/cudasw4_amd_mask.h over the host library.

Needs no GPU, like stats.py: the scalar statement of the rule in libcudasw4_host.so (swdrv_mask_threshold, swdrv_mask_subject).
The database itself is masked on the device: Driver.set_subject_masking, capi.mask_subjects.
"""
import numpy as np

from . import driver as _driver

DEFAULT_WINDOW = 12
DEFAULT_TRIGGER_BITS = 1.9
DEFAULT_EXTEND_BITS = 2.2
MIN_WINDOW, MAX_WINDOW = 4, 32
MASK_CODE = 20


def threshold(window, bits):
    """max(1, ceil(1024 W (log2 W - bits))): the sum S a window of W letters reaches at `bits` of Shannon entropy."""
    if not MIN_WINDOW <= int(window) <= MAX_WINDOW:
        raise ValueError("the window must lie in [%d, %d]" % (MIN_WINDOW, MAX_WINDOW))
    return int(_driver._mask_fns()[2](int(window), float(bits)))


def mask_subject(codes, window=DEFAULT_WINDOW, trigger_bits=DEFAULT_TRIGGER_BITS, extend_bits=DEFAULT_EXTEND_BITS,
                 trigger_sum=None, extend_sum=None, with_count=False):
    """The masked copy of one subject's codes (int8): positions of masked segments become code 20.  The thresholds come from
    the entropies in bits, or directly as sums.  with_count: -> (codes, positions covered by the segments)."""
    c = np.ascontiguousarray(codes, dtype=np.int8)
    ts = threshold(window, trigger_bits) if trigger_sum is None else int(trigger_sum)
    es = threshold(window, extend_bits) if extend_sum is None else int(extend_sum)
    out = np.empty_like(c)
    n = int(_driver._mask_fns()[3](c.ctypes.data, len(c), int(window), ts, es, out.ctypes.data))
    if n < 0:
        raise ValueError("window 4 .. 32 and 1 <= extend sum <= trigger sum are required")
    return (out, n) if with_count else out
