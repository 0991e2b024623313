"""The query-anchored MSA of a query's hits and its redundancy filter, restated in numpy / plain Python from the
definition (include/cudasw4_amd_msa.h).  TEST INFRASTRUCTURE ONLY: independent of cudasw4_amd/msa.py and of
the kernels — a scalar walk per hit, a double loop for the greedy filter."""
import numpy as np

GAP, NONE = 21, 22
OK = 0
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
FIELDS = ["score", "status", "q_begin", "q_end", "s_begin", "s_end", "columns", "identities", "mismatches", "gap_opens",
          "gap_columns", "cigar_len"]
RECORD = np.dtype([(f, np.int32) for f in FIELDS] + [("cigar_offset", np.int64)])   # the layout of sw_align_result


def takes_part(rec, include, h):
    if include is not None and int(include[h]) == 0:
        return False
    return int(rec["status"]) == OK and int(rec["cigar_len"]) > 0


def hit_row(qlen, subject, rec, words):
    """one hit's row from its record, its CIGAR words and its subject codes (the hit takes part)"""
    row = np.full(qlen, NONE, dtype=np.uint8)
    i, j = int(rec["q_begin"]), int(rec["s_begin"])
    if i < 0 or j < 0:
        return row
    q_end, slen = int(rec["q_end"]), len(subject)
    for w in words:
        if i >= qlen:
            break
        length, op = int(w) >> 4, int(w) & 15
        if op in (OP_EQ, OP_X):
            for ii in range(i, min(i + length, qlen)):
                jj = j + (ii - i)
                if 0 <= jj < slen:
                    a = int(subject[jj]) & 0xFF
                    row[ii] = a if a < 20 else 20
            i += length
            j += length
        elif op == OP_I:
            for ii in range(i, min(i + length, qlen, q_end)):
                row[ii] = GAP
            i += length
        elif op == OP_D:
            j += length
    return row


def build_rows(query, qlen, chars, offsets, lengths, results, cigar, include=None):
    """-> (n + 1, qlen) uint8, row n the master"""
    n = len(results)
    rows = np.full((n + 1, qlen), NONE, dtype=np.uint8)
    for h in range(n):
        rec = results[h]
        if not takes_part(rec, include, h):
            continue
        at = int(offsets[h]) - int(offsets[0])
        subject = np.asarray(chars[at:at + int(lengths[h])])
        off, m = int(rec["cigar_offset"]), int(rec["cigar_len"])
        rows[h] = hit_row(qlen, subject, rec, cigar[off:off + m])
    if query is not None:
        q = np.asarray(query).astype(np.int64) & 0xFF
        rows[n] = np.where(q < 20, q, 20).astype(np.uint8)
    return rows


def residues(rows):
    return (rows < 20).sum(axis=1).astype(np.int32)


def ident(row_g, row_h):
    return int(((row_g == row_h) & (row_h < 20)).sum())


def greedy_order(n):
    """row indices in the order of the filter: the master (row n) first"""
    return [n] + list(range(n))


def pair_ident(rows):
    """(n + 1, n + 1) uint32: [h][g] = ident(g, h) for every g before h in the greedy order, 0 elsewhere"""
    n = len(rows) - 1
    out = np.zeros((n + 1, n + 1), dtype=np.uint32)
    order = greedy_order(n)
    for k, h in enumerate(order):
        for g in order[:k]:
            out[h, g] = ident(rows[g], rows[h])
    return out


def pair_ident_onehot(rows):
    """the same through one-hot matrix products (exact in float64 far beyond any qlen here)"""
    n = len(rows) - 1
    hot = np.zeros((n + 1, rows.shape[1], 20), dtype=np.float64)
    for a in range(20):
        hot[:, :, a] = rows == a
    flat = hot.reshape(n + 1, -1)
    full = np.rint(flat @ flat.T).astype(np.uint32)   # [h][g], symmetric: equal residues at equal positions
    out = np.zeros_like(full)
    out[:n, n] = full[:n, n]
    out[:n, :n] = np.tril(full[:n, :n], -1)
    return out


def similar(ident_gh, res_h, P):
    return res_h > 0 and 100 * int(ident_gh) >= P * int(res_h)


def greedy(rows, P, idents=None):
    """-> (keep (n + 1) uint8, purged).  idents: pair_ident(rows) when the caller has it already"""
    n = len(rows) - 1
    res = residues(rows)
    keep = np.zeros(n + 1, dtype=np.uint8)
    purged = 0
    kept = []
    for h in greedy_order(n):
        if res[h] == 0:
            continue
        if P > 0 and h != n:
            red = False
            for g in kept:
                v = idents[h, g] if idents is not None else ident(rows[g], rows[h])
                if similar(v, res[h], P):
                    red = True
                    break
            if red:
                purged += 1
                continue
        keep[h] = 1
        kept.append(h)
    return keep, purged


def msa_filter(query, qlen, chars, offsets, lengths, results, cigar, include, P, with_ident=True):
    rows = build_rows(query, qlen, chars, offsets, lengths, results, cigar, include)
    idents = pair_ident(rows) if with_ident else None
    keep, purged = greedy(rows, P, idents)
    return dict(rows=rows, residues=residues(rows), keep=keep, purged=purged, pair_ident=idents)


# ---- formatting, from the layout in the issue ---------------------------------------------------------------------------

def a3m_line(qlen, subject_letters, rec, words, fasta=False):
    out = ["-"] * int(rec["q_begin"])
    j = int(rec["s_begin"])
    for w in words:
        length, op = int(w) >> 4, int(w) & 15
        if op in (OP_EQ, OP_X):
            out.append(subject_letters[j:j + length].upper())
            j += length
        elif op == OP_I:
            out.append("-" * length)
        elif op == OP_D:
            if not fasta:
                out.append(subject_letters[j:j + length].lower())
            j += length
    line = "".join(out)
    have = sum(1 for c in line if c == "-" or c.isupper())
    return line + "-" * (qlen - have)


def cigar_words(text):
    """'12=1X3I' -> words"""
    ops = {"I": OP_I, "D": OP_D, "=": OP_EQ, "X": OP_X}
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append(int(num) << 4 | ops[ch])
            num = ""
    return np.array(out, dtype=np.uint32)


# ---- random valid inputs ---------------------------------------------------------------------------------------------

def random_case(rng, qlen, n, max_runs=12, other_rate=0.02, no_part_rate=0.1, families=0, copy_rate=0.03):
    """random subjects and random VALID CIGARs with consistent records -> dict of the C ABI's host arrays.
    families > 0: the aligned residues of hit h are a noisy copy of one of `families` parent rows, so that the filter has
    something to purge."""
    query = rng.integers(0, 21, qlen).astype(np.int8)
    parents = [rng.integers(0, 20, qlen).astype(np.int8) for _ in range(families)]
    subjects, recs, words_all = [], np.zeros(n, dtype=RECORD), []
    at = 5   # (the CIGAR buffer starts with a gap: cigar_offset is what locates a hit's words)
    for h in range(n):
        qb = int(rng.integers(0, qlen))
        span = int(rng.integers(1, qlen - qb + 1))
        # split the query span into runs of '=' / 'X' / 'I', with 'D' runs in between
        runs, left = [], span
        want = int(rng.integers(1, max_runs + 1))
        while left > 0:
            length = left if len(runs) >= want - 1 else int(rng.integers(1, max(2, left // max(1, want - len(runs)) * 2)))
            length = min(length, left)
            op = [OP_EQ, OP_X, OP_I][int(rng.integers(0, 3))] if runs else OP_EQ
            if left - length == 0 and op == OP_I:
                op = OP_X
            if runs and runs[-1][1] == op:
                op = OP_X if op != OP_X else OP_EQ
            runs.append((length, op))
            left -= length
            if left > 0 and rng.random() < 0.3 and op != OP_I:
                runs.append((int(rng.integers(1, 6)), OP_D))
        sb = int(rng.integers(0, 8))
        s_need = sb + sum(l for l, op in runs if op != OP_I)
        subject = rng.integers(0, 20, s_need + int(rng.integers(0, 8))).astype(np.int8)
        if families:
            parent = parents[int(rng.integers(0, families))]
            i, j = qb, sb
            for l, op in runs:
                if op in (OP_EQ, OP_X):
                    subject[j:j + l] = parent[i:i + l]
                if op != OP_D:
                    i += l
                if op != OP_I:
                    j += l
            flip = rng.random(len(subject)) < copy_rate
            subject[flip] = rng.integers(0, 20, int(flip.sum()))
        other = rng.random(len(subject)) < other_rate
        subject[other] = 20
        subjects.append(subject)
        w = np.array([l << 4 | op for l, op in runs], dtype=np.uint32)
        r = recs[h]
        r["status"], r["q_begin"], r["q_end"], r["s_begin"] = OK, qb, qb + span, sb
        r["s_end"] = s_need
        r["cigar_len"], r["cigar_offset"] = len(w), at
        u = rng.random()
        if no_part_rate > 0 and n >= 8 and h in (3, 6):   # (enough hits: both kinds are there whatever the draw)
            u = 0.0 if h == 3 else no_part_rate * 0.75
        if u < no_part_rate / 2:
            r["status"] = 2
        elif u < no_part_rate:
            r["cigar_len"] = 0
        words_all.append(w)
        at += len(w) + int(rng.integers(0, 3))
    cigar = np.full(at + 4, 0xFFFFFFFF, dtype=np.uint32)
    for h in range(n):
        cigar[int(recs[h]["cigar_offset"]):int(recs[h]["cigar_offset"]) + len(words_all[h])] = words_all[h]
    lengths = np.array([len(s) for s in subjects], dtype=np.int32)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lengths)
    chars = np.concatenate(subjects + [np.zeros(4, dtype=np.int8)]) if n else np.zeros(4, dtype=np.int8)
    return dict(query=query, qlen=qlen, n=n, chars=chars, offsets=offsets, lengths=lengths, results=recs, cigar=cigar)
