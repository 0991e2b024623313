"""GPU: randomised soak of sw_align_hsps / sw_align_hsps_pssm against the scalar reference tests/hsp_ref.c: small random
queries with planted repeats (hsp_cases.random_case: queries up to 600, subjects up to 900, max_hsps 1 .. 5, random gap
scores and min_score), both score sources.  The seed of a failing case is in the assertion message."""
import numpy as np
import pytest

import gpu_util as G
import hsp_abi as HA
import hsp_cases as HC

pytestmark = pytest.mark.gpu

CASES_PER_BLOCK = 50


@pytest.fixture(scope="module")
def env():
    torch, capi, _ = G.gpu_modules()
    ctx = capi.Context(0)
    yield torch, capi, ctx
    ctx.close()


@pytest.mark.parametrize("block", range(6))
def test_random_cases(env, block):
    for k in range(CASES_PER_BLOCK):
        seed = [8300, block, k]
        rng = np.random.default_rng(seed)
        c = HC.random_case(rng)
        form = HC.FORMS[(block + k) % 3]
        case = HC.make_case(c["q"], form, c["which"])
        where = ("seed", seed, form, c["gop"], c["gex"], c["max_hsps"], c["min_score"])
        call = HA.run(*env, case, c["subjects"], c["gop"], c["gex"], c["max_hsps"], c["min_score"])
        want = HA.want_of(case, c["subjects"], c["gop"], c["gex"], c["max_hsps"], c["min_score"])
        bad = HA.check(call, want, where)
        assert bad is None, bad
        for i, s in enumerate(c["subjects"]):
            bad = HC.check_properties(case, s, c["gop"], c["gex"], want[i * c["max_hsps"]:(i + 1) * c["max_hsps"]])
            assert bad is None, (bad, where, i)
