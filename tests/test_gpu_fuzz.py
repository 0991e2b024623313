"""GPU: a short pass of the randomised soak test (tests/fuzz_gpu.py): random DB shapes, queries around every stripe /
group-shape boundary, gap scores, matrices incl. the 25-letter tables, kernel-type configurations, both host drivers,
resident and streamed, int32 native and in fp32 lanes — every score and every top-10 list against the CPU oracle.
FUZZ_SECONDS / FUZZ_SEED lengthen or reseed it (the long runs are recorded in profiles/r02_results.md)."""
import os

import pytest

pytestmark = pytest.mark.gpu


def test_randomised_soak_short(monkeypatch):
    import fuzz_gpu
    for var in ("CUDASW4_AMD_I32_NATIVE", "CUDASW4_AMD_LANES8_MAX_Q", "CUDASW4_AMD_STREAM", "CUDASW4_AMD_GRID_CAP"):
        monkeypatch.setenv(var, os.environ.get(var, "-1" if "LANES8" in var else "0"))  # restored after the test
    seconds = os.environ.get("FUZZ_SECONDS", "25")
    seed = os.environ.get("FUZZ_SEED", "314")
    cases = fuzz_gpu.main(["--seconds", seconds, "--seed", seed, "--driver-bias", "0.3"])
    assert cases >= 20


def test_randomised_soak_align_short():
    """40 cases of `--features align`: hit alignment of letter and PSSM queries through the C ABI (random budgets, CIGAR
    slots, scratch sizes, expected scores, gap scores up to the documented bound) and, one case in three, the host driver.
    MI355X: 0.9 s inside the suite, 3.0 s as the first GPU test of a process."""
    import fuzz_gpu
    seed = os.environ.get("FUZZ_SEED", "2718")
    assert fuzz_gpu.main(["--features", "align", "--cases", "40", "--seed", seed]) == 40


def test_randomised_soak_pssm_short():
    """30 cases of `--features pssm`: profile search through both hosts under the hooks, every score and the top 10.
    MI355X: 2.1 s inside the suite, 3.8 s as the first GPU test of a process."""
    import fuzz_gpu
    seed = os.environ.get("FUZZ_SEED", "1618")
    assert fuzz_gpu.main(["--features", "pssm", "--cases", "30", "--seed", seed]) == 30
