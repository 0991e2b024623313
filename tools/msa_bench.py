#!/usr/bin/env python3
"""MSA filter timing (sw_msa_filter): HIP-event times of its three stages (rows, pairs, greedy) for the top-500 and the
top-16384 hits of the 464-residue golden query on the Swiss-Prot-like synthetic DB, next to sw_align_hits of the same hits
and to the numpy restatement of the pair stage (cudasw4_amd.msa.pair_identity) on the same rows.  Medians of --reps runs.
Prints one JSON line.

    python tools/msa_bench.py [--n 570000] [--tops 500,16384] [--reps 5] [--identity 90] [--host-rows 4096]

The numpy pair stage is quadratic: above --host-rows rows it is timed on the first --host-rows rows and scaled by the number
of pairs (the line says which: host_pair_rows_timed)."""
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


def one_top(torch, capi, msa, ctx, q, chars, offsets, lengths, result, reps, identity, host_rows):
    ids, scores = result["ids"], result["scores"]
    subjects = [chars[int(offsets[i]):int(offsets[i]) + int(lengths[i])] for i in ids]
    n, qlen = len(subjects), len(q)
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
    drows = torch.zeros((n + 1) * qlen, dtype=torch.uint8, device="cuda")
    dresid = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    dkeep = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
    dpurged = torch.zeros(1, dtype=torch.int32, device="cuda")
    filt = lambda **kw: capi.msa_filter(ctx, dq.data_ptr(), qlen, n, dch.data_ptr(), doff.data_ptr(), dlen.data_ptr(), dres.data_ptr(),
                                        dcig.data_ptr(), 0, identity, dresid.data_ptr(), dkeep.data_ptr(), dpurged.data_ptr(),
                                        rows=drows.data_ptr(), **kw)
    mneed = filt()
    mtemp = torch.empty(mneed, dtype=torch.uint8, device="cuda")
    aev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    mev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for e in aev + mev:
        e.record()
    torch.cuda.synchronize()
    align_ms, msa_ms = [], []
    for _ in range(reps + 1):   # (the first pass warms up and is dropped)
        align(temp=temp.data_ptr(), temp_bytes=need, phase_events=[int(e.cuda_event) for e in aev])
        filt(temp=mtemp.data_ptr(), temp_bytes=mneed, phase_events=[int(e.cuda_event) for e in mev])
        torch.cuda.synchronize()
        align_ms.append(aev[0].elapsed_time(aev[3]))
        msa_ms.append([mev[i].elapsed_time(mev[i + 1]) for i in range(3)])
    align_ms = float(np.median(align_ms[1:]))
    msa_ms = np.median(np.array(msa_ms[1:]), axis=0).tolist()
    rows = drows.cpu().numpy().reshape(n + 1, qlen)
    keep = dkeep.cpu().numpy()
    # the host restatement of the pair stage on the same rows (the master last, as the module wants it)
    m = min(n, host_rows)
    part = np.concatenate([rows[:m], rows[n:]])
    t0 = time.perf_counter()
    idents = msa.pair_identity(part)
    host_s = time.perf_counter() - t0
    pairs = lambda k: k * (k + 1) // 2
    host_full_s = host_s * pairs(n) / max(pairs(m), 1)
    hkeep, hpurged = msa.greedy_keep(part, identity, idents)
    if m == n:
        assert hkeep.tolist() == keep.tolist() and hpurged == int(dpurged.item())
    words = (qlen + 31) // 32
    return {"hits": n, "temp_bytes": mneed, "kept": int(keep[:n].sum()), "purged": int(dpurged.item()),
            "rows_ms": round(msa_ms[0], 4), "pairs_ms": round(msa_ms[1], 4), "greedy_ms": round(msa_ms[2], 4),
            "align_hits_ms": round(align_ms, 4), "pairs_over_align": round(msa_ms[1] / align_ms, 5),
            "pair_words": pairs(n) * words, "pairs_ns_per_pair_word": round(msa_ms[1] * 1e6 / max(pairs(n) * words, 1), 5),
            "host_pair_rows_timed": m, "host_pairs_s_timed": round(host_s, 4), "host_pairs_s": round(host_full_s, 3),
            "host_over_device_pairs": round(host_full_s * 1e3 / msa_ms[1], 1)}


def main():
    from cudasw4_amd import synthdb
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=synthdb.SPROT_SEQUENCES)
    ap.add_argument("--tops", default="500,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--qlen", type=int, default=464)
    ap.add_argument("--identity", type=int, default=90)
    ap.add_argument("--host-rows", type=int, default=4096)
    args = ap.parse_args()
    import torch
    from cudasw4_amd import capi, driver, msa
    chars, offsets, lengths = synthdb.sprot_like(args.n)
    _, letters = driver.read_sequences(os.path.join(ROOT, "tests", "golden", "allqueries.fasta"))
    q_letters = [x for x in letters if len(x) == args.qlen][0]
    q = driver.encode(q_letters)
    tops = [int(t) for t in args.tops.split(",")]
    d = driver.Driver(devices=[0], num_top=max(tops), kinds=(0, 0, 3, 3))
    d.db_from_arrays(chars, offsets, lengths)
    d.upload()
    full = d.scan(q_letters)
    d.close()
    ctx = capi.Context(0)
    ctx.set_matrix(driver.matrix(62))
    out = {"metric": "msa_filter", "db_sequences": int(len(lengths)), "qlen": len(q), "reps": args.reps, "identity": args.identity}
    for top in tops:
        result = {"ids": full["ids"][:top], "scores": full["scores"][:top]}
        out["top%d" % top] = one_top(torch, capi, msa, ctx, q, chars, offsets, lengths, result, args.reps, args.identity, args.host_rows)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
