"""The query-anchored multiple alignment of a query's aligned hits on the host: the rows, their pairwise
identity, the greedy redundancy filter and the A3M / FASTA text.  Needs no GPU and no native library — this is the host
restatement of sw_msa_filter (include/cudasw4_amd_msa.h) that tools/msa_bench.py times the kernels against, and what a
caller without a device can run on alignments it already has."""
import numpy as np

GAP, NONE = 21, 22
_OPS = {"I": 1, "D": 2, "=": 7, "X": 8}


def cigar_words(cigar):
    """a CIGAR string ('12=1X3I', '*' for none) or an array of len << 4 | op words -> uint32 words"""
    if not isinstance(cigar, str):
        return np.asarray(cigar, dtype=np.uint32)
    if cigar in ("", "*"):
        return np.zeros(0, dtype=np.uint32)
    out, num = [], 0
    for ch in cigar:
        if ch.isdigit():
            num = num * 10 + int(ch)
        else:
            out.append(num << 4 | _OPS[ch])
            num = 0
    return np.array(out, dtype=np.uint32)


def rows_from_alignments(query, subjects, results, cigars, include=None):
    """query: master codes (qlen) — or an int, qlen alone, for no master row; subjects: one code array per hit; results: the
    hits' records (anything indexable by field name: status, q_begin, q_end, s_begin, cigar_len); cigars: one CIGAR per hit
    (string or words).  -> (n + 1, qlen) uint8, row n the master."""
    qlen = int(query) if np.isscalar(query) else len(query)
    n = len(subjects)
    rows = np.full((n + 1, qlen), NONE, dtype=np.uint8)
    if not np.isscalar(query):
        q = np.asarray(query).astype(np.int64) & 0xFF
        rows[n] = np.minimum(q, 20)
    for h in range(n):
        r = results[h]
        words = cigar_words(cigars[h])
        if (include is not None and not include[h]) or int(r["status"]) != 0 or int(r["cigar_len"]) <= 0 or len(words) == 0:
            continue
        i, j, q_end = int(r["q_begin"]), int(r["s_begin"]), int(r["q_end"])
        if i < 0 or j < 0:
            continue
        s = np.asarray(subjects[h]).astype(np.int64) & 0xFF
        row = rows[h]
        for w in words:
            if i >= qlen:
                break
            length, op = int(w) >> 4, int(w) & 15
            if op in (7, 8):
                m = max(0, min(length, qlen - i, len(s) - j))   # (a run that leaves the subject: NONE beyond it)
                row[i:i + m] = np.minimum(s[j:j + m], 20)
                i += length
                j += length
            elif op == 1:
                row[i:max(i, min(i + length, qlen, q_end))] = GAP
                i += length
            elif op == 2:
                j += length
    return rows


def pair_identity(rows):
    """(n + 1, n + 1) uint32: [h][g] = #{i: rows[g][i] == rows[h][i] < 20} for every g before h in the filter's order (the
    master, row n, before every hit; hit g before hit h > g), 0 elsewhere"""
    rows = np.asarray(rows, dtype=np.uint8)
    n = len(rows) - 1
    out = np.zeros((n + 1, n + 1), dtype=np.uint32)
    for h in range(n):
        valid = rows[h] < 20
        cols = np.flatnonzero(valid)
        if len(cols) == 0:
            continue
        mine = rows[h, cols]
        out[h, :h] = (rows[:h][:, cols] == mine).sum(axis=1)
        out[h, n] = int((rows[n, cols] == mine).sum())
    return out


def greedy_keep(rows, max_identity, idents=None):
    """the greedy filter at max_identity per cent (0: none) -> (keep (n + 1) uint8, purged)"""
    rows = np.asarray(rows, dtype=np.uint8)
    P = int(max_identity)
    if not 0 <= P <= 100:
        raise ValueError("max_identity must lie in [0, 100]")
    n = len(rows) - 1
    res = (rows < 20).sum(axis=1).astype(np.int64)
    keep = np.zeros(n + 1, dtype=np.uint8)
    keep[n] = res[n] > 0
    if P == 0:
        keep[:n] = res[:n] > 0
        return keep, 0
    if idents is None:
        idents = pair_identity(rows)
    purged = 0
    for h in range(n):
        if res[h] == 0:
            continue
        earlier = np.flatnonzero(keep[:h])
        red = bool((100 * idents[h, earlier].astype(np.int64) >= P * res[h]).any())
        if not red and keep[n]:
            red = 100 * int(idents[h, n]) >= P * int(res[h])
        if red:
            purged += 1
        else:
            keep[h] = 1
    return keep, purged


STATE_NONE, STATE_KEPT, STATE_COVERAGE, STATE_QUERY_IDENTITY, STATE_THINNED = 0, 1, 2, 3, 4


def check_ladder(ladder):
    """-> the rungs as a list of ints: 1 .. 16 strictly ascending values in 1 .. 100"""
    rungs = [int(p) for p in ladder]
    if not 1 <= len(rungs) <= 16:
        raise ValueError("the ladder needs 1 .. 16 rungs")
    if any(not 1 <= p <= 100 for p in rungs) or any(b <= a for a, b in zip(rungs, rungs[1:])):
        raise ValueError("the rungs must lie in [1, 100] and ascend strictly")
    return rungs


def default_ladder(last=90):
    """the rungs `align --msaDiff` uses without --msaDiffLadder: 20, 30, ... below `last`, then `last`"""
    return [p for p in range(20, 100, 10) if p < last] + [int(last)]


def select_rows(rows, min_coverage=0, min_query_identity=0, diff=0, ladder=(90,)):
    """the selection of sw_msa_select on rows ((n + 1, qlen) uint8, row n the master): a hit must have
    min_coverage per cent of the query's positions aligned and be min_query_identity per cent identical to the master; the
    rest are candidates, taken rung by rung of the ascending identity `ladder` in rank order: a candidate is kept when some
    column of it still has fewer than `diff` kept residues (diff 0: always) and no kept row is similar to it at the rung.
    -> (state (n + 1) uint8: 0 none, 1 kept, 2 below coverage, 3 below query identity, 4 thinned; depth (qlen) int32;
    counts [kept hits, below coverage, below query identity, thinned]).
    One pass over all rows per kept row: the time grows with kept rows x rows x qlen."""
    rows = np.asarray(rows, dtype=np.uint8)
    C, Q, D = int(min_coverage), int(min_query_identity), int(diff)
    rungs = np.array(check_ladder(ladder), dtype=np.int64)
    if not 0 <= C <= 100 or not 0 <= Q <= 100 or D < 0:
        raise ValueError("min_coverage and min_query_identity must lie in [0, 100], diff must not be negative")
    n, qlen = len(rows) - 1, rows.shape[1]
    valid = rows < 20
    res = valid.sum(axis=1).astype(np.int64)
    state = np.zeros(n + 1, dtype=np.uint8)
    depth = np.zeros(qlen, dtype=np.int32)
    maxlev = np.zeros(n + 1, dtype=np.int64)   # the most rungs at which a kept row is similar to the row

    def ident_to(g):
        return ((rows == rows[g]) & valid).sum(axis=1).astype(np.int64)

    def keep(g):
        state[g] = STATE_KEPT
        depth[valid[g]] += 1
        similar = (100 * ident_to(g))[:, None] >= rungs[None, :] * res[:, None]
        level = np.where(res > 0, similar.sum(axis=1), 0)
        level[g] = 0
        np.maximum(maxlev, level, out=maxlev)

    candidates = []
    if res[n] > 0:
        keep(n)
    to_master = ident_to(n) if Q > 0 else None
    aligned = (rows <= 20).sum(axis=1).astype(np.int64)
    for h in range(n):
        if res[h] == 0:
            continue
        if 100 * aligned[h] < C * qlen:
            state[h] = STATE_COVERAGE
        elif Q > 0 and 100 * to_master[h] < Q * res[h]:
            state[h] = STATE_QUERY_IDENTITY
        else:
            state[h] = STATE_THINNED
            candidates.append(h)
    for t in range(len(rungs)):
        left = []
        for h in candidates:
            if D > 0 and not (depth[valid[h]] < D).any():
                continue   # not needed now, so never again: depth only grows
            if maxlev[h] > t:
                left.append(h)
                continue
            keep(h)
        candidates = left
    counts = [int((state[:n] == s).sum()) for s in (STATE_KEPT, STATE_COVERAGE, STATE_QUERY_IDENTITY, STATE_THINNED)]
    return state, depth, counts


def format_a3m(query_letters, query_header, headers, subject_letters, results, cigars, keep=None, fmt="a3m"):
    """the text `align --outMsa` writes: the master, then every kept hit in rank order.  subject_letters: the hits' RAW
    letters; '=' / 'X' columns print them in upper case, 'I' columns '-', 'D' runs the letters in lower case (fmt 'fasta':
    not at all); '-' before q_begin and up to qlen."""
    if fmt not in ("a3m", "fasta"):
        raise ValueError("fmt must be 'a3m' or 'fasta'")
    qlen = len(query_letters)
    out = [">" + query_header, query_letters]
    for h in range(len(headers)):
        r = results[h]
        words = cigar_words(cigars[h])
        if (keep is not None and not keep[h]) or int(r["status"]) != 0 or len(words) == 0:
            continue
        s = "".join(c if c.isalpha() else "X" for c in subject_letters[h])   # (a gap character is no residue: 'X')
        line, j = ["-" * int(r["q_begin"])], int(r["s_begin"])
        used = int(r["q_begin"])
        for w in words:
            length, op = int(w) >> 4, int(w) & 15
            if op in (7, 8):
                line.append(s[j:j + length].upper())
                j += length
                used += length
            elif op == 1:
                line.append("-" * length)
                used += length
            elif op == 2:
                if fmt == "a3m":
                    line.append(s[j:j + length].lower())
                j += length
        line.append("-" * (qlen - used))
        out += [">" + headers[h], "".join(line)]
    return "\n".join(out) + "\n"
