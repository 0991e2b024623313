"""Planted inputs of the PSSM-building tests: a query and subjects per case, and what the case is there for as a predicate
over the alignment records (checked on the CPU against align_ref in test_pssm_build_cases_cpu.py, and on the GPU against
what sw_align_hits wrote in test_gpu_pssm_build.py).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

OTHER = 20


def flank(n):
    return np.full(n, OTHER, dtype=np.int8)   # letters no row scores above zero: the alignment stays inside


def mutate_every_other(q):
    s = q.copy()
    s[1::2] = (s[1::2] + 7) % 20
    return s


def copies_with_indels(rng, q, n):
    """relatives with substitutions, short insertions and deletions"""
    out = []
    for _ in range(n):
        copy = []
        for c in q:
            r = rng.random()
            if r < 0.05:
                continue
            if r < 0.10:
                copy.extend(rng.integers(0, 20, int(rng.integers(1, 4))).tolist())
            copy.append(int(rng.integers(0, 20)) if r > 0.8 else int(c))
        out.append(np.concatenate([rng.integers(0, 20, int(rng.integers(0, 9))).astype(np.int8), np.array(copy, dtype=np.int8),
                                   rng.integers(0, 20, int(rng.integers(0, 9))).astype(np.int8)]))
    return out


def ops_of(words):
    return [int(w) & 15 for w in words]


def max_run(words, ops=(7, 8)):
    return max([int(w) >> 4 for w in words if (int(w) & 15) in ops] or [0])


def _all_ok(res, cig):
    return all(int(r["status"]) == 0 and int(r["cigar_len"]) > 0 for r in res)


def cases():
    """-> list of dicts: name, q (codes), subjects (list of code arrays), gop, gex, holds(res, cig) -> bool, where res is
    the record array and cig the list of every hit's CIGAR words"""
    out = []
    rng = np.random.default_rng(2024)

    def add(name, q, subjects, holds, gop=-11, gex=-1):
        out.append(dict(name=name, q=np.asarray(q, dtype=np.int8), subjects=subjects, gop=gop, gex=gex, holds=holds))

    # qlen 1: one column at most
    q = np.array([17], dtype=np.int8)
    add("qlen1", q, [np.array([3, 17, 5], dtype=np.int8), np.array([17], dtype=np.int8), np.array([4, 4], dtype=np.int8)],
        lambda res, cig: [int(r["status"]) for r in res] == [0, 0, 1] and int(res[0]["s_begin"]) == 1)
    # around one wave of columns
    for qlen in (63, 64, 65):
        q = rng.integers(0, 20, qlen).astype(np.int8)
        subjects = [q.copy(), mutate_every_other(q)] + copies_with_indels(rng, q, 4)
        add("qlen%d" % qlen, q, subjects,
            lambda res, cig, qlen=qlen: _all_ok(res, cig) and int(res[0]["columns"]) == qlen and len(cig[1]) >= qlen - 3)
    # qlen 600: fragments that start inside the query and off the dword grid of the subject; single runs over 64 and 128
    q = rng.integers(0, 20, 600).astype(np.int8)
    subjects = [np.concatenate([flank(5), q[37:300], flank(3)]),     # one '=' run of 263 columns, s_begin 5
                np.concatenate([flank(2), q[411:481], flank(9)]),    # ... of 70, s_begin 2
                np.concatenate([flank(7), q[100:250], rng.integers(0, 20, 12).astype(np.int8), q[250:400]])]
    subjects += copies_with_indels(rng, q, 3) + copies_with_indels(rng, q[200:420], 2)
    add("qlen600", q, subjects,
        lambda res, cig: _all_ok(res, cig) and [int(r["q_begin"]) for r in res[:3]] == [37, 411, 100]
        and [int(r["s_begin"]) % 4 for r in res[:3]] == [1, 2, 3] and max_run(cig[0]) == 263 and 64 < max_run(cig[1]) <= 128
        and any(o == 2 for o in ops_of(cig[2])))
    # more than 64 and more than 128 runs: '=' and 'X' alternate
    for qlen, least in ((100, 65), (200, 129)):
        q = rng.integers(0, 20, qlen).astype(np.int8)
        add("runs%d" % least, q, [mutate_every_other(q), q.copy()] + copies_with_indels(rng, q, 2),
            lambda res, cig, least=least: _all_ok(res, cig) and len(cig[0]) >= least
            and (least > 128 or len(cig[0]) <= 128) and max_run(cig[0]) <= 2)
    # gaps as cheap as anything: a mismatch turns into an 'I' run next to a 'D' run
    q = rng.integers(0, 20, 90).astype(np.int8)
    s = q.copy()
    s[10::9] = (s[10::9] + 9) % 20
    add("adjacent_gaps", q, [s] + copies_with_indels(rng, q, 3),
        lambda res, cig: _all_ok(res, cig) and any({a, b} == {1, 2} for w in cig for a, b in zip(ops_of(w), ops_of(w)[1:])),
        gop=-1, gex=-1)
    # codes of 20 on both sides: 'other' letters inside aligned columns of the subjects, and in the master
    q = rng.integers(0, 20, 150).astype(np.int8)
    q[5::13] = OTHER
    subjects = []
    for k in range(4):
        s = np.where(q < 20, q, rng.integers(0, 20, len(q))).astype(np.int8)
        s[7 + k::17] = OTHER
        subjects.append(s)
    add("other_codes", q, subjects,
        lambda res, cig: _all_ok(res, cig) and all(int(r["columns"]) > 120 and int(r["gap_columns"]) == 0 for r in res))
    # 300 copies of one subject: every add lands on the same addresses
    q = rng.integers(0, 20, 80).astype(np.int8)
    s = np.concatenate([flank(3), q[4:70]])
    add("copies300", q, [s.copy() for _ in range(300)],
        lambda res, cig: _all_ok(res, cig) and all(int(r["q_begin"]) == 4 and int(r["q_end"]) == 70 for r in res))
    # a hit without an alignment among others; n == 1
    q = rng.integers(0, 20, 70).astype(np.int8)
    add("empty_status", q, [q[10:60].copy(), flank(30), mutate_every_other(q)],
        lambda res, cig: [int(r["status"]) for r in res] == [0, 1, 0] and int(res[1]["cigar_len"]) == 0)
    add("one_hit", q, [q[3:66].copy()], lambda res, cig: _all_ok(res, cig))
    return out
