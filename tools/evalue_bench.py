#!/usr/bin/env python3
"""Cost of the search statistics on the Swiss-Prot-like synthetic DB and the 464-residue golden query:
HIP-event times of sw_score_histogram alone and of sw_topk (k = 10) on the same scores — each launch sequence repeated
`--batch` times between two events, medians of `--reps` after a warm-up —, and the whole scan through the host driver with
the statistics off and on (alternating, medians of the driver's own per-query seconds).  Prints one JSON line.

    python tools/evalue_bench.py [--n 570000] [--reps 5] [--batch 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    from cudasw4_amd import synthdb
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=synthdb.SPROT_SEQUENCES)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--qlen", type=int, default=464)
    ap.add_argument("--k", type=int, default=10)
    args = ap.parse_args()
    import torch
    from cudasw4_amd import capi, driver, stats
    assert torch.cuda.is_available(), "evalue_bench needs a GPU"
    chars, offsets, lengths = synthdb.sprot_like(args.n)
    _, letters = driver.read_sequences(os.path.join(ROOT, "tests", "golden", "allqueries.fasta"))
    q = [x for x in letters if len(x) == args.qlen][0]
    d = driver.Driver(devices=[0], num_top=args.k)
    d.db_from_arrays(chars, offsets, lengths)
    d.upload()
    # the whole scan, statistics off and on, alternating
    scan_ms = {False: [], True: []}
    for rep in range(args.reps + 1):   # (the first pass warms up and is dropped)
        for on in (False, True):
            d.set_statistics(on)
            r = d.scan(q)
            if rep:
                scan_ms[on].append(r["seconds"] * 1e3)
    fit = {k: v for k, v in r["stats"].items() if k not in ("hist", "sumlen")}
    table = r["stats"]["hist"]
    scores, ids = d.last_scores(0)     # shard order: ascending length, as the kernels see them
    d.close()
    n = len(scores)

    ctx = capi.Context(0)
    ds = torch.from_numpy(scores.astype(np.float32)).cuda()
    dl = torch.from_numpy(np.ascontiguousarray(lengths[ids], dtype=np.int32)).cuda()
    di = torch.arange(n, dtype=torch.int32, device="cuda")
    hist = torch.zeros(stats.LBINS * stats.SBINS, dtype=torch.int32, device="cuda")
    sumlen = torch.zeros(stats.LBINS, dtype=torch.int64, device="cuda")
    skipped = torch.zeros(1, dtype=torch.int32, device="cuda")
    tb = capi.topk_temp_bytes(n, args.k)
    temp = torch.empty(max(tb, 1), dtype=torch.uint8, device="cuda")
    os_, oi = torch.zeros(args.k, dtype=torch.float32, device="cuda"), torch.zeros(args.k, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def histogram():
        capi.score_histogram(ctx, ds.data_ptr(), dl.data_ptr(), n, hist.data_ptr(), sumlen.data_ptr(), skipped.data_ptr(), stream)

    def topk():
        ctx.topk(ds.data_ptr(), di.data_ptr(), n, args.k, os_.data_ptr(), oi.data_ptr(), temp.data_ptr(), tb, stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = []
        for rep in range(args.reps + 1):
            e0.record()
            for _ in range(args.batch):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                out.append(e0.elapsed_time(e1) * 1e3 / args.batch)
        return float(np.median(out)), [round(x, 2) for x in out]

    hist_us, hist_all = timed(histogram)
    topk_us, topk_all = timed(topk)
    # the table the timed launches summed is the scan's, once per launch
    launches = (args.reps + 1) * args.batch
    assert np.array_equal(hist.cpu().numpy().view(np.uint32).reshape(table.shape).astype(np.uint64), table.astype(np.uint64) * launches)
    ctx.close()
    off, on = float(np.median(scan_ms[False])), float(np.median(scan_ms[True]))
    print(json.dumps({"metric": "evalue_bench", "db_sequences": n, "qlen": args.qlen, "k": args.k, "reps": args.reps, "batch": args.batch,
                      "score_histogram_us": round(hist_us, 2), "score_histogram_us_all": hist_all,
                      "topk_us": round(topk_us, 2), "topk_us_all": topk_all,
                      "histogram_over_topk": round(hist_us / topk_us, 4),
                      "scan_ms_statistics_off": round(off, 4), "scan_ms_statistics_on": round(on, 4),
                      "scan_ms_off_all": [round(x, 4) for x in scan_ms[False]], "scan_ms_on_all": [round(x, 4) for x in scan_ms[True]],
                      "statistics_cost_ms": round(on - off, 4), "nonzero_cells": int((table > 0).sum()), "fit": fit}))


if __name__ == "__main__":
    main()
