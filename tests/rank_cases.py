"""The inputs the ranking tests share (test_rank_cpu.py, test_gpu_rank.py): the small Swiss-Prot-like DB scored by the CPU
oracle for two golden queries, with the fit and the reference lists.  Computed once per process and never changed."""
import functools

import numpy as np

import oracle_lib as O
import rank_ref as K
import stats_ref as R

# (golden query, k): the pairs of the issue's table that the GPU tests rely on
CASES = ((9, 10), (4, 50))
MAX_EVALUE = 10.0


@functools.lru_cache(maxsize=1)
def small_db():
    from cudasw4_amd import synthdb
    chars, offsets, lengths, family = synthdb.sprot_like(n=3000, max_len=8000, return_family_ids=True)
    _, letters = O.read_fasta(O.GOLDEN_DIR + "/allqueries.fasta")
    _, qs = O.load_queries()
    lengths = np.asarray(lengths)
    want = {}
    for qi, k in CASES:
        sc = O.scan(qs[qi], chars, offsets, lengths, simd=True).astype(np.int64)
        hist, sumlen, skipped = R.histogram(sc, lengths)
        assert skipped == 0
        fit = R.fit(hist, sumlen)
        ids, z = K.ranked(fit, sc, lengths, k)
        want[qi] = {"k": k, "scores": sc, "hist": hist, "sumlen": sumlen, "fit": fit, "z": K.zscores(fit, sc, lengths),
                    "ranked_ids": ids, "ranked_z": z, "count": K.count(fit, sc, lengths, MAX_EVALUE),
                    "z_min": K.z_min(fit["N"], MAX_EVALUE)}
    return {"db": (chars, offsets, lengths), "lengths": lengths, "letters": letters, "codes": qs, "want": want}
