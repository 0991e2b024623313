#!/usr/bin/env python3
"""Hit alignment timing (sw_align_hits): per-phase HIP-event times, aligned cells per second and align time against scan
time for the top-10 and top-100 hits of golden queries (144, 464, 1000, 5478 residues) on the Swiss-Prot-like synthetic
DB, and the longest subject (35 213 residues) against the 5478-residue query alone.  Prints one JSON line.

--pssm: the same queries, hits and scan times, but every alignment through the PSSM form (sw_align_hits_pssm,
swdrv_align_hits_pssm) with pssm.from_sequence(query, table) as the PSSM and the query as the consensus: the same results
(checked against the scan's scores), so the two legs time the two score sources of one step loop.

    python tools/align_hits_bench.py [--n 570000] [--reps 3] [--pssm]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def dbdata(subjects):
    lengths = np.array([len(s) for s in subjects], dtype=np.int32)
    padded = (lengths.astype(np.int64) + 3) // 4 * 4
    offsets = np.zeros(len(subjects) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(padded)
    chars = np.full(int(offsets[-1]), 20, dtype=np.int8)
    for i, s in enumerate(subjects):
        chars[int(offsets[i]):int(offsets[i]) + len(s)] = s
    return chars, offsets, lengths


def time_align(torch, capi, ctx, q, subjects, scores, reps, pssm=None):
    """-> per-phase milliseconds (median over reps), the cells each phase covered, the results.
    pssm: None (sw_align_hits) or the (len(q), 21) PSSM of q (sw_align_hits_pssm, q as the consensus)"""
    chars, offsets, lengths = dbdata(subjects)
    n = len(subjects)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    coff = np.zeros(n + 1, dtype=np.int64)
    coff[1:] = np.cumsum(len(q) + lengths.astype(np.int64))
    dq, dch, doff, dlen, dcoff, dexp = dev(q), dev(chars), dev(offsets), dev(lengths), dev(coff), dev(np.asarray(scores, np.int32))
    dt = capi.align_result_dtype()
    dres = torch.zeros(n * dt.itemsize, dtype=torch.uint8, device="cuda")
    dcig = torch.zeros(int(coff[-1]), dtype=torch.int32, device="cuda")
    tb = max(capi.align_trace_bytes(len(q), int(L)) for L in lengths)
    common = (dq.data_ptr(), len(q), n, dch.data_ptr(), doff.data_ptr(), dlen.data_ptr(), int(lengths.max()), -11, -1, dres.data_ptr(),
              dcig.data_ptr(), dcoff.data_ptr())
    if pssm is None:
        call = lambda **kw: capi.align_hits(ctx, *common, expected_scores=dexp.data_ptr(), trace_bytes=tb, **kw)
    else:
        dp = dev(np.ascontiguousarray(pssm, dtype=np.int8).reshape(-1))
        call = lambda **kw: capi.align_hits_pssm(ctx, dp.data_ptr(), *common, expected_scores=dexp.data_ptr(), trace_bytes=tb, **kw)
    need = call()
    temp = torch.empty(need, dtype=torch.uint8, device="cuda")
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for e in evs:
        e.record()
    torch.cuda.synchronize()
    handles = [int(e.cuda_event) for e in evs]
    times = []
    for _ in range(reps):
        call(temp=temp.data_ptr(), temp_bytes=need, phase_events=handles)
        torch.cuda.synchronize()
        times.append([evs[i].elapsed_time(evs[i + 1]) for i in range(3)])
    ms = np.median(np.array(times), axis=0).tolist()
    res = np.frombuffer(dres.cpu().numpy().tobytes(), dtype=dt).copy()
    assert (res["status"] == capi.ALIGN_OK).all(), res["status"]
    cells_a = float(len(q)) * float(lengths.sum())
    cells_b = float(np.sum(res["q_end"].astype(np.float64) * res["s_end"]))
    cells_c = float(np.sum((res["q_end"] - res["q_begin"]).astype(np.float64) * (res["s_end"] - res["s_begin"])))
    return ms, (cells_a, cells_b, cells_c), res


def main():
    from cudasw4_amd import synthdb
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=synthdb.SPROT_SEQUENCES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pssm", action="store_true", help="align through the PSSM form (from_sequence PSSMs of the same queries)")
    args = ap.parse_args()
    import torch
    from cudasw4_amd import capi, driver, pssm
    table = driver.matrix(62)
    as_pssm = lambda q: pssm.from_sequence(q, table) if args.pssm else None
    chars, offsets, lengths = synthdb.sprot_like(args.n)
    _, letters = driver.read_sequences(os.path.join(ROOT, "tests", "golden", "allqueries.fasta"))
    d = driver.Driver(devices=[0], num_top=100, kinds=(0, 0, 3, 3))
    d.db_from_arrays(chars, offsets, lengths)
    d.upload()
    ctx = capi.Context(0)
    ctx.set_matrix(table)
    subject = lambda i: chars[int(offsets[i]):int(offsets[i]) + int(lengths[i])]
    out = {"metric": "align_hits_pssm" if args.pssm else "align_hits", "db_sequences": int(len(lengths)), "reps": args.reps, "queries": []}
    for q_letters in letters:
        if len(q_letters) not in (144, 464, 1000, 5478):
            continue
        q = driver.encode(q_letters)
        d.scan(q_letters)
        scan_ms = []
        for _ in range(args.reps):
            r = d.scan(q_letters)
            scan_ms.append(r["seconds"] * 1e3)
        entry = {"qlen": len(q), "scan_ms": float(np.median(scan_ms))}
        for top in (10, 100):
            ids, scores = r["ids"][:top], r["scores"][:top]
            ms, cells, _ = time_align(torch, capi, ctx, q, [subject(i) for i in ids], scores, args.reps, pssm=as_pssm(q))
            t0 = time.perf_counter()
            if args.pssm:
                d.align_hits_pssm(as_pssm(q), {"ids": ids, "scores": scores}, consensus=q_letters)
            else:
                d.align_hits(q_letters, {"ids": ids, "scores": scores})
            host_ms = (time.perf_counter() - t0) * 1e3
            total = sum(ms)
            entry["top%d" % top] = {"phase_ms": [round(x, 3) for x in ms], "align_ms": round(total, 3),
                                    "cells": cells, "gcups": round(sum(cells) / (total * 1e-3) / 1e9, 3),
                                    "align_over_scan": round(total / entry["scan_ms"], 4),
                                    "driver_call_ms": round(host_ms, 3)}
        out["queries"].append(entry)
    # the longest subject against the 5478-residue query alone
    giant = int(np.argmax(lengths))
    q = driver.encode([x for x in letters if len(x) == 5478][0])
    s = subject(giant)
    ms, cells, res = time_align(torch, capi, ctx, q, [s], [time_score(ctx, capi, torch, q, s)], args.reps, pssm=as_pssm(q))
    out["giant_pair"] = {"qlen": len(q), "slen": int(len(s)), "phase_ms": [round(x, 3) for x in ms], "align_ms": round(sum(ms), 3),
                         "cells": cells, "gcups": round(sum(cells) / (sum(ms) * 1e-3) / 1e9, 3), "score": int(res[0]["score"])}
    d.close()
    ctx.close()
    print(json.dumps(out))


def time_score(ctx, capi, torch, q, s):
    """the pair's score from a coordinates-only call (the expected score of the timed run)"""
    chars, offsets, lengths = dbdata([s])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dq, dch, doff, dlen = dev(q), dev(chars), dev(offsets), dev(lengths)
    dt = capi.align_result_dtype()
    dres = torch.zeros(dt.itemsize, dtype=torch.uint8, device="cuda")
    args = (dq.data_ptr(), len(q), 1, dch.data_ptr(), doff.data_ptr(), dlen.data_ptr(), int(len(s)), -11, -1, dres.data_ptr())
    need = capi.align_hits(ctx, *args, flags=capi.ALIGN_COORDS_ONLY)
    temp = torch.empty(need, dtype=torch.uint8, device="cuda")
    capi.align_hits(ctx, *args, flags=capi.ALIGN_COORDS_ONLY, temp=temp.data_ptr(), temp_bytes=need)
    torch.cuda.synchronize()
    return int(np.frombuffer(dres.cpu().numpy().tobytes(), dtype=dt)[0]["score"])


if __name__ == "__main__":
    main()
