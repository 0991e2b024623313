#!/usr/bin/env python3
"""PSSM building timing (sw_pssm_accumulate): HIP-event times of the two accumulate launches (memsets and counting; weighting)
next to the three alignment phases of the same hits — the top-500 of the 464-residue golden query on the Swiss-Prot-like
synthetic DB —, and the host time of the conversion (pssm.from_counts).  Prints one JSON line.

    python tools/pssm_build_bench.py [--n 570000] [--top 500] [--reps 5]
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


def main():
    from cudasw4_amd import synthdb
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=synthdb.SPROT_SEQUENCES)
    ap.add_argument("--top", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--qlen", type=int, default=464)
    args = ap.parse_args()
    import torch
    from cudasw4_amd import capi, driver, pssm
    table = driver.matrix(62)
    chars, offsets, lengths = synthdb.sprot_like(args.n)
    _, letters = driver.read_sequences(os.path.join(ROOT, "tests", "golden", "allqueries.fasta"))
    q_letters = [x for x in letters if len(x) == args.qlen][0]
    q = driver.encode(q_letters)
    d = driver.Driver(devices=[0], num_top=args.top, kinds=(0, 0, 3, 3))
    d.db_from_arrays(chars, offsets, lengths)
    d.upload()
    r = d.scan(q_letters)
    t0 = time.perf_counter()
    _, info = d.build_pssm(q_letters, r, min_score=0)
    driver_call_ms = (time.perf_counter() - t0) * 1e3
    d.close()
    ids, scores = r["ids"], r["scores"]
    subjects = [chars[int(offsets[i]):int(offsets[i]) + int(lengths[i])] for i in ids]
    n, qlen = len(subjects), len(q)

    ctx = capi.Context(0)
    ctx.set_matrix(table)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    hc, ho, hl = dbdata(subjects)
    coff = np.zeros(n + 1, dtype=np.int64)
    coff[1:] = np.cumsum(qlen + hl.astype(np.int64))
    dq, dch, doff, dlen, dcoff, dexp = dev(q), dev(hc), dev(ho), dev(hl), dev(coff), dev(np.asarray(scores, np.int32))
    dt = capi.align_result_dtype()
    dres = torch.zeros(n * dt.itemsize, dtype=torch.uint8, device="cuda")
    dcig = torch.zeros(int(coff[-1]), dtype=torch.int32, device="cuda")
    tb = max(capi.align_trace_bytes(qlen, int(L)) for L in hl)
    align = lambda **kw: capi.align_hits(ctx, dq.data_ptr(), qlen, n, dch.data_ptr(), doff.data_ptr(), dlen.data_ptr(), int(hl.max()),
                                         -11, -1, dres.data_ptr(), dcig.data_ptr(), dcoff.data_ptr(), expected_scores=dexp.data_ptr(),
                                         trace_bytes=tb, **kw)
    need = align()
    temp = torch.empty(need, dtype=torch.uint8, device="cuda")
    dcounts = torch.zeros(qlen * 20, dtype=torch.int32, device="cuda")
    dweights = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    dwcounts = torch.zeros(qlen * 20, dtype=torch.int64, device="cuda")
    dused = torch.zeros(1, dtype=torch.int32, device="cuda")
    aev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    bev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for e in aev + bev:
        e.record()
    torch.cuda.synchronize()
    align_ms, acc_ms = [], []
    for _ in range(args.reps + 1):   # (the first pass warms up and is dropped)
        align(temp=temp.data_ptr(), temp_bytes=need, phase_events=[int(e.cuda_event) for e in aev])
        capi.pssm_accumulate(ctx, dq.data_ptr(), qlen, n, dch.data_ptr(), doff.data_ptr(), dlen.data_ptr(), dres.data_ptr(),
                             dcig.data_ptr(), 0, dcounts.data_ptr(), dweights.data_ptr(), dwcounts.data_ptr(), dused.data_ptr(),
                             phase_events=[int(e.cuda_event) for e in bev])
        torch.cuda.synchronize()
        align_ms.append([aev[i].elapsed_time(aev[i + 1]) for i in range(3)])
        acc_ms.append([bev[i].elapsed_time(bev[i + 1]) for i in range(2)])
    align_ms = np.median(np.array(align_ms[1:]), axis=0).tolist()
    acc_ms = np.median(np.array(acc_ms[1:]), axis=0).tolist()
    counts = dcounts.cpu().numpy().view(np.uint32).reshape(qlen, 20)
    wcounts = dwcounts.cpu().numpy().view(np.uint64).reshape(qlen, 20)
    res = np.frombuffer(dres.cpu().numpy().tobytes(), dtype=dt)
    conv = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        p, lam = pssm.from_counts(q, counts, wcounts, matrix=62)
        conv.append((time.perf_counter() - t0) * 1e3)
    # (every hit takes part here; the driver's step leaves copies of the query out, so its PSSM is this one only without them)
    out = {"metric": "pssm_build", "db_sequences": int(len(lengths)), "qlen": qlen, "hits": n, "reps": args.reps,
           "used": int(dused.item()), "aligned_columns": int(res["identities"].sum() + res["mismatches"].sum()),
           "cigar_words": int(res["cigar_len"].sum()), "max_count": int(counts.max()),
           "align_phase_ms": [round(x, 4) for x in align_ms], "align_ms": round(sum(align_ms), 4),
           "accumulate_launch_ms": [round(x, 4) for x in acc_ms], "accumulate_ms": round(sum(acc_ms), 4),
           "accumulate_over_align": round(sum(acc_ms) / sum(align_ms), 5),
           "convert_host_ms": round(float(np.median(conv)), 4), "driver_build_pssm_call_ms": round(driver_call_ms, 3),
           "driver_used": info["used"], "lambda": round(lam, 6)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
