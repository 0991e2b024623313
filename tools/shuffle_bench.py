#!/usr/bin/env python3
"""Cost of the statistics calibrated on shuffled subjects on the Swiss-Prot-like synthetic DB and the
464-residue golden query: HIP-event times of sw_shuffle_subjects alone on the calibration's sample and of the scan of that
sample (SW_KIND_I32, the calibrator's launches) — each launch sequence repeated `--batch` times between two events, medians
of `--reps` after a warm-up —, the whole Driver.calibrate() (host clock around the call: install, shuffle, scans, histogram,
copy back, fit) and the whole scan of the same query through the host driver.  Prints one JSON line.

    python tools/shuffle_bench.py [--n 570000] [--reps 5] [--batch 10] [--subjects 10000] [--shuffles R]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    from cudasw4_amd import synthdb
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=synthdb.SPROT_SEQUENCES)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--qlen", type=int, default=464)
    ap.add_argument("--subjects", type=int, default=10000)
    ap.add_argument("--shuffles", type=int, default=None)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    import torch
    from cudasw4_amd import capi, driver, stats
    assert torch.cuda.is_available(), "shuffle_bench needs a GPU"
    chars, offsets, lengths = synthdb.sprot_like(args.n)
    _, letters = driver.read_sequences(os.path.join(ROOT, "tests", "golden", "allqueries.fasta"))
    q = [x for x in letters if len(x) == args.qlen][0]
    d = driver.Driver(devices=[0], num_top=10)
    d.db_from_arrays(chars, offsets, lengths)
    d.upload()
    d.set_statistics(True)
    scan_ms, cal_ms = [], []
    for rep in range(args.reps + 1):   # (the first pass warms up — and gathers the sample — and is dropped)
        r = d.scan(q)
        t0 = time.perf_counter()
        cal = d.calibrate(q, shuffles=args.shuffles, max_subjects=args.subjects, seed=args.seed)
        t1 = time.perf_counter()
        if rep:
            scan_ms.append(r["seconds"] * 1e3)
            cal_ms.append((t1 - t0) * 1e3)
    scan_fit = {k: v for k, v in r["stats"].items() if k not in ("hist", "sumlen")}
    cal_fit = {k: v for k, v in cal.items() if k not in ("hist", "sumlen")}
    d.close()

    # the sample as the calibrator holds it, and its launches
    ids = stats.shuffle_sample(len(lengths), args.subjects)
    m, reps = len(ids), stats.shuffle_replicas(len(ids), args.shuffles)
    off = np.asarray(offsets).astype(np.int64)
    ls = np.ascontiguousarray(np.asarray(lengths)[ids], dtype=np.int32)
    so = np.zeros(m + 1, dtype=np.int64)
    so[1:] = np.cumsum((ls.astype(np.int64) + 3) // 4 * 4)
    sc = np.full(int(so[-1]), 20, dtype=np.int8)
    for j, i in enumerate(ids):
        sc[so[j]:so[j] + ls[j]] = chars[off[i]:off[i] + ls[j]]
    nbytes = int(so[-1])
    stride = (nbytes + 255) // 256 * 256
    i1, i2 = int(np.searchsorted(ls, 1280, side="right")), int(np.searchsorted(ls, 8000, side="right"))
    merge = i2 - i1 >= 512
    ranges = ([(35, i2, m)] if i2 < m else []) + ([(34, i1, i2)] if not merge and i1 < i2 else []) + \
             ([(33, 0, i2 if merge else i1)] if (i2 if merge else i1) > 0 else [])

    ctx = capi.Context(0)
    ctx.set_matrix(driver.matrix(62))
    ctx.set_query(driver.encode(q))
    dc = torch.from_numpy(sc.view(np.uint8)).cuda()
    do = torch.from_numpy(so).cuda()
    dl = torch.from_numpy(ls).cuda()
    dk = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).cuda()
    out = torch.zeros(stride * reps, dtype=torch.uint8, device="cuda")
    scores = torch.zeros(m * reps, dtype=torch.float32, device="cuda")
    sids = torch.zeros(m * reps, dtype=torch.int32, device="cuda")
    need = max([ctx.scan_temp_bytes(capi.KIND_I32, p, e - b, int(ls[e - 1])) for p, b, e in ranges] + [256])
    temp = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def shuffle():
        capi.shuffle_subjects(ctx, dc.data_ptr(), do.data_ptr(), dl.data_ptr(), m, args.seed, out.data_ptr(), stride,
                              keys=dk.data_ptr(), replicas=reps, stream=stream)

    def scan():
        for r_ in range(reps):
            for p, b, e in ranges:
                ctx.scan_partition(capi.KIND_I32, p, out.data_ptr() + r_ * stride, do.data_ptr(), dl.data_ptr(), b, e - b, int(ls[e - 1]),
                                   -11, -1, scores.data_ptr() + 4 * r_ * m, sids.data_ptr() + 4 * r_ * m, temp=temp.data_ptr(),
                                   temp_bytes=need, stream=stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        res = []
        for rep in range(args.reps + 1):
            e0.record()
            for _ in range(args.batch):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                res.append(e0.elapsed_time(e1) * 1e3 / args.batch)
        return float(np.median(res)), [round(x, 2) for x in res]

    shuffle_us, shuffle_all = timed(shuffle)
    scan_us, scan_all = timed(scan)
    # what was timed is what the calibration histograms
    h, s, skipped = np.zeros((stats.LBINS, stats.SBINS), np.int64), np.zeros(stats.LBINS, np.int64), 0
    got = scores.cpu().numpy().astype(np.int64)
    for sc_, l_ in zip(got, np.tile(ls, reps)):
        h[stats.length_bin(int(l_)), min(int(sc_), 255)] += 1
    assert np.array_equal(h, cal["hist"].astype(np.int64)), "the timed scan's scores are not the calibration's"
    ctx.close()
    residues = int(ls.sum()) * reps
    print(json.dumps({"metric": "shuffle_bench", "db_sequences": len(lengths), "qlen": args.qlen, "reps": args.reps, "batch": args.batch,
                      "sample_subjects": m, "replicas": reps, "sample_bytes": nbytes, "shuffled_residues": residues,
                      "shuffle_us": round(shuffle_us, 2), "shuffle_us_all": shuffle_all,
                      "shuffle_gresidues_per_s": round(residues / shuffle_us / 1e3, 3),
                      "sample_scan_us": round(scan_us, 2), "sample_scan_us_all": scan_all,
                      "shuffle_over_sample_scan": round(shuffle_us / scan_us, 4),
                      "calibrate_ms": round(float(np.median(cal_ms)), 4), "calibrate_ms_all": [round(x, 4) for x in cal_ms],
                      "scan_ms": round(float(np.median(scan_ms)), 4), "scan_ms_all": [round(x, 4) for x in scan_ms],
                      "calibrate_over_scan": round(float(np.median(cal_ms)) / float(np.median(scan_ms)), 4),
                      "scan_fit": scan_fit, "calibrated_fit": cal_fit}))


if __name__ == "__main__":
    main()
