"""CPU: the planted inputs of tests/pssm_build_cases.py do what they are there for (under the scalar aligner align_ref), and the
scalar reference of the accumulation keeps the invariants of the definition on them; the library's conversion of their
counts equals the reference's.  No GPU involved."""
import numpy as np
import pytest

import align_ref as A
import oracle_lib as O
import pssm_build_cases as C
import pssm_build_ref as R

CASES = C.cases()


def cpu_records(case):
    table = O.blosum21(62)
    res = np.zeros(len(case["subjects"]), dtype=R.RECORD)
    words, at = [], 0
    for k, s in enumerate(case["subjects"]):
        r, w = A.align(case["q"], s, table, case["gop"], case["gex"])
        for f in R.FIELDS:
            res[k][f] = r[f]
        res[k]["cigar_offset"] = at
        at += len(w)
        words.append(w)
    return res, words


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_is_what_it_is_for(case):
    res, words = cpu_records(case)
    assert case["holds"](res, words), [(int(r["status"]), int(r["q_begin"]), int(r["s_begin"]), A.cigar_string(w)[:60])
                                       for r, w in zip(res[:4], words[:4])]
    q, qlen = case["q"], len(case["q"])
    chars, offsets, lengths = O.make_db(case["subjects"])
    cig = np.concatenate(words + [np.zeros(1, dtype=np.uint32)])
    counts, weights, wcounts, used = R.accumulate(q, qlen, chars, offsets, lengths, res, cig)
    assert used == int(((res["status"] == 0) & (res["cigar_len"] > 0)).sum())
    # every position with a residue hands out 2^32 in all, less the floors' losses (below one unit per term)
    filled = int((counts.sum(axis=1) > 0).sum())
    terms = int(counts.sum())
    total = sum(int(w) for w in weights)
    assert filled * (1 << 32) - terms < total <= filled * (1 << 32)
    assert sum(int(x) for x in wcounts.reshape(-1)) == sum(int(w) * int(n) for w, n in zip(weights, residues_per_sequence(case, res, words)))
    # the product's conversion of these counts (real alignments, not the random ones of test_pssm_build_cpu) against the reference's
    from cudasw4_amd import pssm
    want, wraw, _ = R.convert(O.blosum21(62), q, counts, wcounts)
    got, _, raw = pssm.from_counts(q, counts, wcounts, matrix=62, with_raw=True)
    assert np.abs(raw - wraw).max() < 1e-9
    assert (got == want)[np.abs(np.abs(np.pad(wraw, ((0, 0), (0, 1)))) % 1.0 - 0.5) > 1e-6].all() and (got[:, 20] == want[:, 20]).all()
    if case["name"] == "copies300":
        assert int(counts.max()) == 301 and (counts[4:70].max(axis=1) == 301).all() and len(set(weights[:300].tolist())) == 1


def residues_per_sequence(case, res, words):
    """how many (position, residue) pairs every sequence has, the master last: from the CIGARs alone"""
    out = []
    for k, s in enumerate(case["subjects"]):
        n, j = 0, int(res[k]["s_begin"])
        for w in words[k]:
            length, op = int(w) >> 4, int(w) & 15
            if op in (7, 8):
                n += int((s[j:j + length] < 20).sum())
            if op != 1:
                j += length
        out.append(n)
    return out + [int((case["q"] < 20).sum())]
