#!/usr/bin/env python3
"""Cost of the ranking by E-value on the Swiss-Prot-like synthetic DB: HIP-event times of sw_zscore_keys
alone, of keys + sw_topk + sw_gather_hits, and of sw_topk on the raw scores of the same scan — each launch sequence repeated
`--batch` times between two events, medians of `--reps` after a warm-up —, and the whole scan through the host driver ranked
by E-value against the same driver with the statistics on and ranked by score (alternating, medians of the driver's own
per-query seconds), for every `--qlen`.  Prints one JSON line.

    python tools/rank_bench.py [--n 570000] [--reps 5] [--batch 20] [--qlen 464 144 48]
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
    ap.add_argument("--qlen", type=int, nargs="+", default=[464, 144, 48])
    ap.add_argument("--k", type=int, default=10)
    args = ap.parse_args()
    import torch
    from cudasw4_amd import capi, driver
    assert torch.cuda.is_available(), "rank_bench needs a GPU"
    chars, offsets, lengths = synthdb.sprot_like(args.n)
    _, letters = driver.read_sequences(os.path.join(ROOT, "tests", "golden", "allqueries.fasta"))
    d = driver.Driver(devices=[0], num_top=args.k)
    d.db_from_arrays(chars, offsets, lengths)
    d.upload()
    # the whole scan: statistics on and ranked by score (the path before this mode existed) against ranked by E-value
    scans = {}
    for qlen in args.qlen:
        # the golden query of that length, or a prefix of the longest one
        q = ([x for x in letters if len(x) == qlen] or [max(letters, key=len)[:qlen]])[0]
        ms = {"score": [], "evalue": []}
        differ = 0
        for rep in range(args.reps + 1):   # (the first pass warms up and is dropped)
            lists = {}
            for by in ("score", "evalue"):
                d.set_ranking(by)
                d.set_statistics(True)
                r = d.scan(q)
                lists[by] = r["ids"].tolist()
                if rep:
                    ms[by].append(r["seconds"] * 1e3)
            differ = len(set(lists["evalue"]) - set(lists["score"]))
        s, e = float(np.median(ms["score"])), float(np.median(ms["evalue"]))
        scans[str(qlen)] = {"scan_ms_by_score": round(s, 4), "scan_ms_by_evalue": round(e, 4), "ranking_cost_ms": round(e - s, 4),
                            "by_score_all": [round(x, 4) for x in ms["score"]], "by_evalue_all": [round(x, 4) for x in ms["evalue"]],
                            "subjects_not_in_score_list": differ}
    fit = {k: v for k, v in r["stats"].items() if k not in ("hist", "sumlen")}
    scores, ids = d.last_scores(0)     # shard order: ascending length, as the kernels see them
    d.close()
    n = len(scores)

    ctx = capi.Context(0)
    ds = torch.from_numpy(scores.astype(np.float32)).cuda()
    dl = torch.from_numpy(np.ascontiguousarray(lengths[ids], dtype=np.int32)).cuda()
    di = torch.arange(n, dtype=torch.int32, device="cuda")
    keys = torch.zeros(n, dtype=torch.float32, device="cuda")
    pos = torch.zeros(n, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    tb = capi.topk_temp_bytes(n, args.k)
    temp = torch.empty(max(tb, 1), dtype=torch.uint8, device="cuda")
    tk, tp = torch.zeros(args.k, dtype=torch.float32, device="cuda"), torch.zeros(args.k, dtype=torch.int32, device="cuda")
    os_, oi = torch.zeros(args.k, dtype=torch.float32, device="cuda"), torch.zeros(args.k, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    no_threshold = -sys.float_info.max

    def make_keys():
        capi.zscore_keys(ctx, ds.data_ptr(), dl.data_ptr(), n, fit["a"], fit["b1"], fit["sd"], no_threshold, keys.data_ptr(), pos.data_ptr(),
                         count.data_ptr(), stream)

    def ranked():
        make_keys()
        ctx.topk(keys.data_ptr(), pos.data_ptr(), n, args.k, tk.data_ptr(), tp.data_ptr(), temp.data_ptr(), tb, stream)
        capi.gather_hits(ctx, tp.data_ptr(), args.k, ds.data_ptr(), di.data_ptr(), os_.data_ptr(), oi.data_ptr(), stream)

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

    keys_us, keys_all = timed(make_keys)
    ranked_us, ranked_all = timed(ranked)
    topk_us, topk_all = timed(topk)
    # every timed launch counted every scored subject once
    launches = 2 * (args.reps + 1) * args.batch
    assert int(count.cpu()[0]) == launches * int((scores >= 0).sum())
    ctx.close()
    print(json.dumps({"metric": "rank_bench", "db_sequences": n, "k": args.k, "reps": args.reps, "batch": args.batch,
                      "zscore_keys_us": round(keys_us, 2), "zscore_keys_us_all": keys_all,
                      "zscore_keys_gb_per_s": round(16.0 * n / keys_us / 1e3, 1),
                      "keys_topk_gather_us": round(ranked_us, 2), "keys_topk_gather_us_all": ranked_all,
                      "topk_raw_scores_us": round(topk_us, 2), "topk_raw_scores_us_all": topk_all,
                      "ranked_over_topk": round(ranked_us / topk_us, 4), "scans": scans, "fit_of_last_query": fit}))


if __name__ == "__main__":
    main()
