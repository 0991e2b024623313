"""Case builders of the tests of sw_align_hsps / sw_align_hsps_pssm (several alignments per hit).  TEST INFRASTRUCTURE ONLY:
numpy and the scalar reference (hsp_ref), no GPU.

A case is an align_cases.Case (letters, or the PSSM of the same letters: pssm.from_sequence with the letters as the caller's
consensus, so both forms have the same records) plus its subjects.  Nothing here knows an expected result: the tests
compare with hsp_ref, and check the properties every set of alignments has (monotone scores, disjoint pairs, rescoring,
positive end columns) on top."""
import numpy as np

import align_cases as C
import hsp_ref as H
import oracle_lib as O

FORMS = ["letters", "pssm", "pssm-argmax"]


def make_case(q, form="letters", which=62):
    """the query q under BLOSUM `which`: as letters, as its PSSM with q as the consensus, or as its PSSM without one"""
    q = np.ascontiguousarray(q, dtype=np.int8)
    table, mref = C.matrix_rows(which, False)
    if form == "letters":
        return C.Case(q=q, table=table, mref=mref)
    from cudasw4_amd import pssm
    return C.Case(pssm=pssm.from_sequence(q, table), consensus=q.copy() if form == "pssm" else None)


def reference(case, s, gop, gex, max_hsps, min_score, **kw):
    """hsp_ref's slots [(fields, words)] for one subject (kw: expected, trace_bytes, caps, max_subject_len)"""
    s = np.minimum(np.asarray(s, dtype=np.int8).view(np.uint8), 20).astype(np.int8)   # what the kernels read
    if case.is_pssm:
        return H.align(case.consensus, s, pssm=case.pssm, gop=gop, gex=gex, max_hsps=max_hsps, min_score=min_score, **kw)
    return H.align(case.q, s, m=case.mref, gop=gop, gex=gex, max_hsps=max_hsps, min_score=min_score, **kw)


def plain_scores(case):
    """(qlen x 21) scores without any veto"""
    return np.asarray(case.pssm if case.is_pssm else np.asarray(case.mref).reshape(-1, 21)[case.q], dtype=np.int64)


def check_properties(case, s, gop, gex, slots):
    """what holds for the alignments of one hit whatever the tie rules.  -> None, or what is wrong"""
    s = np.minimum(np.asarray(s, dtype=np.int8).view(np.uint8), 20).astype(np.int8)
    sc = plain_scores(case)
    seen, last = set(), None
    for k, (r, w) in enumerate(slots):
        if r["status"] != H.OK:
            continue
        if last is not None and r["score"] > last:
            return "slot %d: score %d above its predecessor's %d" % (k, r["score"], last)
        last = r["score"]
        if case.rescore(s, gop, gex, r, w) != r["score"]:
            return "slot %d: the CIGAR rescored gives %d, not %d" % (k, case.rescore(s, gop, gex, r, w), r["score"])
        ps = H.pairs(r, w)
        if seen & set(ps):
            return "slot %d shares pairs with an earlier alignment: %r" % (k, sorted(seen & set(ps))[:3])
        seen |= set(ps)
        if (int(w[0]) & 15) not in (7, 8) or (int(w[-1]) & 15) not in (7, 8):
            return "slot %d begins or ends with a gap" % k
        if sc[ps[0][0], s[ps[0][1]]] <= 0 or sc[ps[-1][0], s[ps[-1][1]]] <= 0:
            return "slot %d: an end column scores 0 or less" % k
    return None


def spacer(rng, n=10):
    return rng.integers(0, 20, n).astype(np.int8)


def mutated(rng, x, rate=0.12):
    y = np.array(x, dtype=np.int8)
    hit = rng.random(len(y)) < rate
    y[hit] = rng.integers(0, 20, int(hit.sum()))
    return y


def three_copies(rng, qlen=24):
    """-> (q, subject): three exact copies of the query between 10-residue random spacers"""
    q = rng.integers(0, 20, qlen).astype(np.int8)
    return q, np.concatenate([spacer(rng), q, spacer(rng), q, spacer(rng), q, spacer(rng)])


def swapped_domains(rng, la=30, lb=34):
    """-> (q, subject): query = domains A B, subject = B A"""
    a, b = rng.integers(0, 20, la).astype(np.int8), rng.integers(0, 20, lb).astype(np.int8)
    return np.concatenate([a, spacer(rng, 5), b]), np.concatenate([spacer(rng), b, spacer(rng, 7), a, spacer(rng)])


def tandem(rng, unit=23, nq=2, ns=3):
    """-> (q, subject): nq tandem repeats against ns (lightly mutated, so that the copies are told apart by score)"""
    u = rng.integers(0, 20, unit).astype(np.int8)
    q = np.concatenate([u] * nq)
    return q, np.concatenate([spacer(rng, 6)] + [mutated(rng, u, 0.08) for _ in range(ns)] + [spacer(rng, 6)])


def border_subjects(rng, q):
    """Subjects whose earlier alignments leave used pairs in a lane's first and last row, in lane 0 and lane 63, in column 0
    and in the last column, and across rows 511 / 512, at begins and ends that are no multiples of 8 (so that the reverse and
    the trace pass see them at other lane offsets than the local pass):
      0  starts with a copy of the query's head (row 0 x column 0) and ends with a copy of its tail (last row x last column),
         with two copies of an inner piece [a, b) between them (the same rows used twice, in different columns)
      1  the whole query twice, the second copy mutated: alignment 0 runs through every stripe border and every lane
      2  pieces around row 512 when the query has one: [503, min(L, 517)) three times"""
    L = len(q)
    a, b = (1, L - 1) if L < 16 else (3, L - 5)
    head, tail = q[:max(2, min(L, 13) - 2)], q[L - max(2, min(L, 11) - 2):]
    inner = q[a:b]
    subs = [np.concatenate([head, spacer(rng, 9), inner, spacer(rng, 7), mutated(rng, inner, 0.05), spacer(rng, 5), tail]),
            np.concatenate([spacer(rng, 3), q, spacer(rng, 11), mutated(rng, q, 0.1)])]
    if L > 512:
        piece = q[503:min(L, 517)]
        subs.append(np.concatenate([piece, spacer(rng, 4), piece, spacer(rng, 4), piece]))
    return subs


def three_stripes(rng, qlen=1100):
    """-> (q, subject): a query of three stripes with two planted hits, one of them inside the last stripe only"""
    q = rng.integers(0, 20, qlen).astype(np.int8)
    return q, np.concatenate([spacer(rng, 13), q[1037:1093], spacer(rng, 21), mutated(rng, q[301:467], 0.1), spacer(rng, 9)])


def random_case(rng, max_q=600, max_s=900):
    """one random query with planted repeats in 1 .. 4 subjects, random scoring and max_hsps 1 .. 5.
    -> dict(q, subjects, which, gop, gex, max_hsps, min_score)"""
    qlen = int(rng.choice([int(rng.integers(1, 40)), int(rng.integers(40, 200)), int(rng.integers(200, max_q + 1))]))
    q = rng.integers(0, 20, qlen).astype(np.int8)
    subjects = []
    for _ in range(int(rng.integers(1, 5))):
        parts, total = [spacer(rng, int(rng.integers(0, 30)))], 0
        for _ in range(int(rng.integers(1, 5))):
            lo = int(rng.integers(0, qlen))
            hi = int(rng.integers(lo + 1, min(qlen, lo + 250) + 1))
            piece = mutated(rng, q[lo:hi], float(rng.choice([0.0, 0.05, 0.2])))
            if len(piece) > 6 and rng.random() < 0.3:     # a deletion or an insertion inside the copy
                at = int(rng.integers(1, len(piece) - 1))
                piece = np.concatenate([piece[:at], spacer(rng, int(rng.integers(1, 6))), piece[at + int(rng.integers(0, 3)):]])
            parts += [piece, spacer(rng, int(rng.integers(0, 30)))]
        s = np.concatenate(parts)[:max_s]
        if len(s) == 0:
            s = spacer(rng, 5)
        subjects.append(s)
    gop, gex = [(-11, -1), (-11, -1), (-5, -5), (-13, -2), (-2, -5)][int(rng.integers(0, 5))]
    return dict(q=q, subjects=subjects, which=int(rng.choice([62, 50])), gop=gop, gex=gex, max_hsps=int(rng.integers(1, 6)),
                min_score=int(rng.choice([1, 1, 15, 40])))
