"""The two databases of DESIGN.md §15 that the scan's own fit cannot serve, shared by test_shuffle_cpu.py and
test_gpu_shuffle.py: one dominated by a family of weak relatives of golden query 2, and one too small to fit.  Scored once
by the CPU oracle, calibrated once by the numpy restatement (shuffle_ref.py); nothing here calls the library."""
import functools

import numpy as np

import oracle_lib as O
import shuffle_ref as SR
import stats_ref as R

QUERY = 2
SHUFFLE_SEED = 2024
FRAGMENT, SUBSTITUTED = 150, 0.6


def _build(n_unrelated, n_relatives):
    """n_unrelated subjects of sprot_like(3000, families=False), evenly spread over its length order, and n_relatives weak
    relatives of the query: a 150-residue fragment of it, 60 % of the residues substituted, between random flanks.
    -> (chars, offsets, lengths, is_relative), ascending by length."""
    from cudasw4_amd import synthdb
    chars, offsets, lengths = synthdb.sprot_like(n=3000, max_len=8000, families=False)
    _, qs = O.load_queries()
    q = np.asarray(qs[QUERY], dtype=np.int8)
    rng = np.random.default_rng(11)
    seqs, rel = [], []
    for i in np.linspace(0, 2999, n_unrelated).astype(np.int64):
        seqs.append(np.array(chars[int(offsets[i]):int(offsets[i]) + int(lengths[i])], dtype=np.int8))
        rel.append(False)
    for _ in range(n_relatives):
        start = int(rng.integers(0, len(q) - FRAGMENT + 1))
        frag = q[start:start + FRAGMENT].copy()
        hit = rng.random(FRAGMENT) < SUBSTITUTED
        frag[hit] = rng.integers(0, 20, int(hit.sum()), dtype=np.int8)
        left = rng.integers(0, 20, int(rng.integers(10, 200)), dtype=np.int8)
        right = rng.integers(0, 20, int(rng.integers(10, 200)), dtype=np.int8)
        seqs.append(np.concatenate([left, frag, right]))
        rel.append(True)
    order = np.argsort([len(s) for s in seqs], kind="stable")
    seqs = [seqs[i] for i in order]
    rel = np.array(rel)[order]
    c, o, ls = O.make_db(seqs)
    assert (np.diff(ls) >= 0).all()
    return c, o, ls, rel


@functools.lru_cache(maxsize=None)
def case(name):
    """"family": 360 unrelated + 240 relatives, 4 shuffles; "small": 60 unrelated + 3 relatives, 32 shuffles.
    -> dict: the DB, the query (codes and letters), the oracle's scores, the scan's table and fit, the reference calibration
    and the calibrated statistics"""
    n_unrelated, n_relatives, shuffles = {"family": (360, 240, 4), "small": (60, 3, 32)}[name]
    chars, offsets, lengths, rel = _build(n_unrelated, n_relatives)
    _, qs = O.load_queries()
    _, letters = O.read_fasta(__import__("os").path.join(O.GOLDEN_DIR, "allqueries.fasta"))
    q = qs[QUERY]
    scores = O.scan(q, chars, offsets, lengths, simd=True).astype(np.int64)
    hist, sumlen, skipped = R.histogram(scores, lengths)
    assert skipped == 0
    scan_fit = R.fit(hist, sumlen)
    chist, csumlen, cfit, m, reps = SR.calibrate(lambda c, o, l: O.scan(q, c, o, l, simd=True), chars, offsets, lengths,
                                                 SHUFFLE_SEED, shuffles=shuffles)
    assert (m, reps) == (len(lengths), shuffles)
    stats = SR.calibrated(cfit, scan_fit["N"])
    z, e = R.evalues(stats, scores, lengths)
    return {"chars": chars, "offsets": offsets, "lengths": np.asarray(lengths), "relative": rel, "query": q,
            "letters": letters[QUERY], "scores": scores, "scan_fit": scan_fit, "shuffles": shuffles, "cal_hist": chist,
            "cal_sumlen": csumlen, "cal_fit": cfit, "stats": stats, "z": z, "e": e}
