#!/usr/bin/env python3
"""Profile search against the letter query of the same length: what does a PSSM query cost?

    python tools/pssm_bench.py [--passes 3] [--peak 1000000x512] [--sprot 570000] [--letters-only]

For the 20 golden queries on the peak pseudo-DB and on the Swiss-Prot-like synthetic DB: GCUPS of the letter query and of
pssm.from_sequence of the same query, both under the C++ driver's own clock (Driver.scan / Driver.scan_pssm: seconds from
submission to merged top-K), top-K lists compared query by query.  Per DB and leg the tool reports the rate over all
queries (cells / summed seconds) of every pass — median, minimum and maximum over the passes — and per-query medians.
The cost of installing the query (staging + upload + profile build, everything between submission and the first scan
kernel) is measured apart, with HIP events around sw_set_query / sw_set_query_pssm followed by a one-subject scan.

--letters-only runs the letter leg alone: the mode for a build of the library that has no PSSM entry point
(CUDASW4_AMD_LIB / CUDASW4_AMD_HOST_LIB name another build).  Prints ONE JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np


def install_cost_us(letters, m21, reps=20):
    """HIP-event time of installing a query and building its first profile: set_query[_pssm] + a scan of one short subject"""
    import torch
    from cudasw4_amd import capi, pssm, search
    import oracle_lib as O
    seq = [O.encode(b"ACDEFGHIKLMNPQRSTVWY" * 3)]
    chars, offsets, lengths = O.make_db(seq)
    db = search.DeviceDB.from_arrays(chars, offsets, lengths, device=0)
    s = search.Searcher(device=0, num_top=0, matrix=m21)
    s.set_database(db)
    out = {}
    for qlen in (144, 1000, 5478):
        q = next(x for x in letters if len(x) == qlen)
        codes = O.encode(q)
        p = pssm.from_sequence(codes, m21)
        row = {}
        for leg in ("letters", "pssm"):
            if leg == "pssm" and not hasattr(capi.lib, "sw_set_query_pssm"):
                continue
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if leg == "pssm":
                    s.ctx.set_query = lambda c, st=0: capi.Context.set_query_pssm(s.ctx, p, st)
                e0.record()
                s.scan(codes, timed=False, sync=False)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
                if leg == "pssm":
                    del s.ctx.set_query
            row[leg] = round(statistics.median(ts[2:]), 1)
        out[str(qlen)] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--peak", default="1000000x512")
    ap.add_argument("--sprot", type=int, default=570000)
    ap.add_argument("--letters-only", action="store_true")
    ap.add_argument("--top", type=int, default=10)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "pssm_bench needs a GPU"
    from cudasw4_amd import driver, pssm, synthdb
    import oracle_lib as O
    _, letters = O.read_fasta(os.path.join(O.GOLDEN_DIR, "allqueries.fasta"))
    m = driver.matrix(62)
    pssms = [pssm.from_sequence(driver.encode(q), m) for q in letters]
    legs = ["letters"] if args.letters_only else ["letters", "pssm"]
    result = {"tool": "pssm_bench", "passes": args.passes, "legs": legs, "library": os.environ.get("CUDASW4_AMD_LIB", "tree"), "dbs": {}}
    num, length = (int(x) for x in args.peak.split("x"))
    for name in ("peak", "sprot_like"):
        d = driver.Driver(devices=[0], num_top=args.top, kinds=(0, 0, 3, 3))
        if name == "peak":
            d.pseudo_db(num, length)
            residues = float(num) * length
        else:
            chars, offsets, lengths = synthdb.sprot_like(args.sprot)[:3]
            d.db_from_arrays(chars, offsets, lengths)
            residues = float(np.asarray(lengths, dtype=np.int64).sum())
        d.upload()
        tops = {}
        per_pass = {leg: [] for leg in legs}
        per_query = {leg: [[] for _ in letters] for leg in legs}
        for pas in range(args.passes + 1):   # pass 0 warms up (code objects, buffers) and is where the top-K lists are compared
            for leg in legs:
                total = 0.0
                for qi, q in enumerate(letters):
                    r = d.scan(q) if leg == "letters" else d.scan_pssm(pssms[qi])
                    total += r["seconds"]
                    if pas == 0:
                        tops.setdefault(qi, {})[leg] = (r["scores"].tolist(), r["ids"].tolist(), r["num_overflows"])
                    else:
                        per_query[leg][qi].append(len(q) * residues / 1e9 / r["seconds"])
                if pas > 0:
                    per_pass[leg].append(sum(len(q) for q in letters) * residues / 1e9 / total)
        same = all(len(set(map(str, t.values()))) == 1 for t in tops.values())
        entry = {"residues": residues, "topk_equal": bool(same) if len(legs) == 2 else None}
        for leg in legs:
            v = per_pass[leg]
            entry[leg] = {"gcups_median": round(statistics.median(v), 1), "gcups_min": round(min(v), 1), "gcups_max": round(max(v), 1),
                          "per_query_median": [round(statistics.median(x), 1) for x in per_query[leg]]}
        if len(legs) == 2:
            entry["pssm_over_letters"] = round(entry["pssm"]["gcups_median"] / entry["letters"]["gcups_median"], 4)
        result["dbs"][name] = entry
        d.close()
    result["install_us"] = install_cost_us(letters, O.blosum21(62))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
