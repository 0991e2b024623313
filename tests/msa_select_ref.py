"""The selection of MSA rows (coverage, identity to the query, the diversity filter over a ladder of identity thresholds)
restated in plain Python loops from the definition (include/cudasw4_amd_msa_select.h).  TEST INFRASTRUCTURE
ONLY: independent of cudasw4_amd/msa.py and of the kernels.  Rows come from tests/msa_ref.py."""
import numpy as np

import msa_ref as M

NONE, KEPT, COVERAGE, QUERY_IDENTITY, THINNED = 0, 1, 2, 3, 4


def pairs(row):
    return sum(1 for v in row if v <= 20)


def needed(row, depth, D):
    if D == 0:
        return True
    for i, v in enumerate(row):
        if v < 20 and depth[i] < D:
            return True
    return False


def ident_matrix(rows):
    """(n + 1, n + 1): [h][g] = ident(g, h), computed once for the callers below (ident is symmetric: equal codes below 20)"""
    m = len(rows)
    out = np.zeros((m, m), dtype=np.int64)
    for h in range(m):
        for g in range(h):
            out[h, g] = out[g, h] = M.ident(rows[g], rows[h])
    return out


def levels(rows, ladder, idents=None):
    """(n + 1, n + 1) uint8: [h][g] = number of rungs at which g is similar to h, for every ordered pair g != h"""
    m = len(rows)
    res = [sum(1 for v in r if v < 20) for r in rows]
    out = np.zeros((m, m), dtype=np.uint8)
    for h in range(m):
        for g in range(m):
            if g != h:
                v = M.ident(rows[g], rows[h]) if idents is None else int(idents[h, g])
                out[h, g] = sum(1 for P in ladder if M.similar(v, res[h], P))
    return out


def select(rows, C=0, Q=0, D=0, ladder=(90,), trace=None, idents=None):
    """-> (state (n + 1) uint8, depth (qlen) int32, counts [kept hits, below coverage, below query identity, thinned]).
    trace: a list that receives (rung, row) for every hit as it is kept; idents: ident_matrix(rows) when the caller has it."""
    rows = np.asarray(rows)
    ident = (lambda g, h: M.ident(rows[g], rows[h])) if idents is None else (lambda g, h: int(idents[h, g]))
    n, qlen = len(rows) - 1, rows.shape[1]
    res = [sum(1 for v in r if v < 20) for r in rows]
    state = [NONE] * (n + 1)
    depth = [0] * qlen
    kept = []

    def keep(h):
        state[h] = KEPT
        kept.append(h)
        for i in range(qlen):
            if rows[h][i] < 20:
                depth[i] += 1
    if res[n] > 0:
        keep(n)
    candidates = []
    for h in range(n):
        if res[h] == 0:
            continue
        if C > 0 and 100 * pairs(rows[h]) < C * qlen:
            state[h] = COVERAGE
        elif Q > 0 and 100 * ident(n, h) < Q * res[h]:
            state[h] = QUERY_IDENTITY
        else:
            candidates.append(h)
    for t, P in enumerate(ladder):
        for h in list(candidates):
            if not needed(rows[h], depth, D):
                continue
            if any(M.similar(ident(g, h), res[h], P) for g in kept):
                continue
            keep(h)
            candidates.remove(h)
            if trace is not None:
                trace.append((t, h))
    for h in candidates:
        state[h] = THINNED
    counts = [sum(1 for h in range(n) if state[h] == s) for s in (KEPT, COVERAGE, QUERY_IDENTITY, THINNED)]
    return np.array(state, dtype=np.uint8), np.array(depth, dtype=np.int32), counts


def case_rows(case, include=None, with_query=True):
    return M.build_rows(case["query"] if with_query else None, case["qlen"], case["chars"], case["offsets"], case["lengths"],
                        case["results"], case["cigar"], include)


GUARD_CASES = [(33, 65, 2), (70, 130, 3), (129, 200, 4)]
GUARD_SEEDS = (1, 2, 3)
GUARD_PARAMS = dict(C=30, Q=5, D=3, ladder=(20, 40, 60, 80, 95))


def guard_case(qlen, n, families, seed):
    return M.random_case(np.random.default_rng(seed), qlen, n, families=families, copy_rate=0.15)
