"""Position-specific scoring matrices (PSSMs) as queries: construction from a string, NCBI ASCII reader / writer.

A PSSM is a (qlen, 21) int8 array: row i = query position i, column c = dbdata subject code c
(0..19 = ARNDCQEGHILKMFPSTWYV, 20 = "other" and the padding of the dbdata layout; it must be negative in every row).
Pure Python / numpy, but for from_counts (the host library's conversion of aligned hits' counts into a PSSM): the scans
themselves run in the HIP library (capi.Context.set_query_pssm, driver.Driver.scan_pssm).
"""
import numpy as np

LETTERS = "ARNDCQEGHILKMFPSTWYV"   # the NCBI column order is this project's code order 0..19
COLUMNS = 21
OTHER_SCORE = -1                   # what the ASCII reader puts into column 20


class PssmFormatError(ValueError):
    """A malformed PSSM file; the message names file and line."""


def as_pssm(array):
    """-> contiguous (qlen, 21) int8 array, checked against the contract of sw_set_query_pssm."""
    m = np.asarray(array)
    if m.ndim != 2 or m.shape[1] != COLUMNS or m.shape[0] < 1:
        raise ValueError("a PSSM is a (qlen, %d) array with qlen >= 1, got shape %r" % (COLUMNS, m.shape))
    if m.dtype != np.int8:
        if not np.issubdtype(m.dtype, np.integer) or m.min() < -128 or m.max() > 127:
            raise ValueError("PSSM scores must be integers in [-128, 127]")
        m = m.astype(np.int8)
    if (m[:, 20] >= 0).any():
        raise ValueError("column 20 (other / padding) must be negative in every row: row %d is not" % int(np.argmax(m[:, 20] >= 0)))
    return np.ascontiguousarray(m)


def from_sequence(letters, matrix):
    """The PSSM that reproduces a letter query: row i = the substitution table's row of letter i.

    letters: encoded query (codes 0..dim-1, any integer sequence) or a residue string (with a 21-letter table: the 20
             standard residues, everything else = code 20; with a 25-letter table: ARNDCQEGHILKMFPSTWYVBJZX*).
    matrix:  dim x dim table (flat or square), dim = 21 or 25.  Subject codes are the dbdata alphabet 0..20 either way:
             with a 25-letter table subject code 20 is scored with the table's X column, as sw_set_matrix does."""
    m = np.asarray(matrix, dtype=np.int8).reshape(-1)
    dim = int(round(len(m) ** 0.5))
    if dim * dim != len(m) or dim not in (21, 25):
        raise ValueError("substitution tables are 21 x 21 or 25 x 25")
    m = m.reshape(dim, dim)
    if isinstance(letters, (str, bytes)):
        text = letters.decode() if isinstance(letters, bytes) else letters
        alphabet = LETTERS if dim == 21 else LETTERS + "BJZX*"
        other = 20 if dim == 21 else 23
        codes = np.array([alphabet.find(ch) if ch in alphabet else other for ch in text.upper()], dtype=np.int64)
    else:
        codes = np.asarray(letters, dtype=np.int64)
    if codes.ndim != 1 or len(codes) < 1 or codes.min() < 0 or codes.max() >= dim:
        raise ValueError("query codes must be 0..%d" % (dim - 1))
    cols = list(range(20)) + [23 if dim == 25 else 20]
    return as_pssm(m[codes][:, cols])


def from_counts(master, counts, wcounts, matrix=62, pseudocount=10.0, with_raw=False):
    """The PSSM of a master sequence's aligned hits, from their residue counts and weighted counts (what
    capi.pssm_accumulate computes on the GPU; DESIGN.md "Building a PSSM").  A thin binding of the host library's
    swdrv_pssm_from_counts; no GPU needed.

    master: residue string or dbdata codes (20 and above: not a standard residue); counts / wcounts: (qlen, 20) uint32 /
    uint64; matrix: 45 | 50 | 62 | 80 (or the 25-letter 4525 ...: the 21-letter table of the same name); pseudocount > 0.
    -> (pssm, lambda), with_raw: (pssm, lambda, (qlen, 20) float64 scores before rounding)"""
    from . import driver
    if isinstance(master, (str, bytes)):
        master = driver.encode(master)
    return driver.pssm_from_counts(master, counts, wcounts, matrix=matrix, pseudocount=pseudocount, with_raw=with_raw)


def consensus_of(pssm):
    """The best-scoring standard residue of every position (what write_ascii prints when given no consensus)."""
    return "".join(LETTERS[int(i)] for i in np.argmax(np.asarray(pssm)[:, :20], axis=1))


def _is_int(tok):
    t = tok[1:] if tok[:1] in "+-" else tok
    return t.isdigit()


def parse_ascii(lines, name="<pssm>"):
    """-> (pssm, consensus) from the lines of an NCBI ASCII PSSM (psiblast -out_ascii_pssm).

    A header line with the 20 column letters in the order A R N D C Q E G H I L K M F P S T W Y V (once, or twice when
    the percentage block follows), then one line per position: index (consecutive from 1), consensus residue, 20 integer
    scores, optionally 20 percentages and two information columns (ignored).  Parsing stops at the first line behind the
    positions that is not a position line (the Lambda / K footer).  Column 20 is OTHER_SCORE in every row."""
    def bad(lineno, what):
        return PssmFormatError("%s:%d: %s" % (name, lineno, what))
    header = None
    rows, cons = [], []
    last_line = 0
    for lineno, raw in enumerate(lines, 1):
        last_line = lineno
        tok = raw.split()
        if header is None:
            if len(tok) >= 20 and all(len(t) == 1 and t.isalpha() for t in tok):
                if "".join(tok[:20]).upper() != LETTERS or len(tok) not in (20, 40) or (len(tok) == 40 and "".join(tok[20:]).upper() != LETTERS):
                    raise bad(lineno, "column header is not 'A R N D C Q E G H I L K M F P S T W Y V'")
                header = lineno
            elif len(tok) >= 2 and tok[0].isdigit() and len(tok[1]) == 1 and tok[1].isalpha():
                raise bad(lineno, "position line before the column header (missing header)")
            continue
        if not tok:
            if rows:
                break
            continue
        if not (tok[0].isdigit() and len(tok) >= 2 and len(tok[1]) == 1 and (tok[1].isalpha() or tok[1] in "*-")):
            if rows:
                break   # the footer
            raise bad(lineno, "expected a position line (index, residue, 20 scores)")
        if int(tok[0]) != len(rows) + 1:
            raise bad(lineno, "position index %s, expected %d (indices must be consecutive from 1)" % (tok[0], len(rows) + 1))
        vals = tok[2:]
        if len(vals) not in (20, 40, 42) or not all(_is_int(v) for v in vals[:20]):
            raise bad(lineno, "expected 20 integer scores (optionally 20 percentages and 2 information columns), got %d columns" % len(vals))
        sc = [int(v) for v in vals[:20]]
        for v in sc:
            if v < -128 or v > 127:
                raise bad(lineno, "score %d outside the int8 range" % v)
        rows.append(sc + [OTHER_SCORE])
        cons.append(tok[1].upper())
    if header is None:
        raise bad(max(last_line, 1), "no column header 'A R N D C Q E G H I L K M F P S T W Y V' found (missing header)")
    if not rows:
        raise bad(last_line, "no position lines behind the column header")
    return np.array(rows, dtype=np.int8), "".join(cons)


def read_ascii(path):
    """-> (pssm, consensus) of an NCBI ASCII PSSM file; PssmFormatError names file and line."""
    with open(path, "r") as f:
        return parse_ascii(f, name=str(path))


def write_ascii(path, pssm, consensus=None, percentages=False, footer=False):
    """Write the 20 standard columns of `pssm` as an NCBI ASCII PSSM (column 20 is not part of the format).
    percentages / footer: also emit the (zero) percentage and information columns / a Lambda-K footer, as psiblast does."""
    m = np.asarray(pssm)
    if m.ndim != 2 or m.shape[1] not in (20, COLUMNS):
        raise ValueError("a PSSM is a (qlen, 21) array")
    cons = consensus if consensus is not None else consensus_of(m)
    if len(cons) != m.shape[0]:
        raise ValueError("consensus has %d residues, the PSSM %d rows" % (len(cons), m.shape[0]))
    head = "           " + "".join("%5s" % c for c in LETTERS)   # (psiblast: 3 columns per score; 5 keep -128 apart)
    with open(path, "w") as f:
        f.write("\nLast position-specific scoring matrix computed, weighted observed percentages rounded down, "
                "information per position, and relative weight of gapless real matches to pseudocounts\n")
        f.write(head + ("   " + "".join("%4s" % c for c in LETTERS) if percentages else "") + "\n")
        for i in range(m.shape[0]):
            line = "%5d %s  " % (i + 1, cons[i]) + "".join("%5d" % int(v) for v in m[i, :20])
            if percentages:
                line += " " + "".join("%4d" % 0 for _ in range(20)) + "  0.00 0.00"
            f.write(line + "\n")
        if footer:
            f.write("\n                      K         Lambda\n")
            f.write("Standard Ungapped    0.1340     0.3170\n")
            f.write("Standard Gapped      0.0410     0.2670\n")
            f.write("PSI Ungapped         0.1340     0.3170\n")
            f.write("PSI Gapped           0.0410     0.2670\n")
