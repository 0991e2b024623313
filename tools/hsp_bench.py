#!/usr/bin/env python3
"""Timing of several alignments per hit (sw_align_hsps): for the top-10 and top-100 hits of the 144-, 464- and 1000-residue
golden queries on the Swiss-Prot-like synthetic DB, with max_hsps 1, 2, 4 and 8 and min_score 1 (so that every round runs):
the whole call (HIP events around it, median and spread over the repetitions), the time per vetoed round from calls with
successive max_hsps, its ratio to round 0 (the max_hsps = 1 call: the same pairs, the plain kernels) and sw_align_hits
itself on the same pairs.  Prints one JSON line.

--plain-only: only sw_align_hits (runs on a build without sw_align_hsps too: CUDASW4_AMD_LIB=<another build's library>
compares two builds in one session).

    python tools/hsp_bench.py [--n 570000] [--reps 7] [--pssm] [--plain-only]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from tools.align_hits_bench import dbdata  # noqa: E402

HSPS = (1, 2, 4, 8)


def spread(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def time_calls(torch, capi, ctx, q, subjects, scores, reps, pssm, plain_only):
    """-> {"align_hits": spread, "max_hsps": {m: spread + slots}} of one set of pairs"""
    chars, offsets, lengths = dbdata(subjects)
    n, qlen = len(subjects), len(q)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dq, dch, doff, dlen, dexp = dev(q), dev(chars), dev(offsets), dev(lengths), dev(np.asarray(scores, np.int32))
    dp = dev(np.ascontiguousarray(pssm, dtype=np.int8).reshape(-1)) if pssm is not None else None
    dt = capi.align_result_dtype()
    tb = max(capi.align_trace_bytes(qlen, int(L)) for L in lengths)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(m, hsps):
        coff = np.zeros(n * m + 1, dtype=np.int64)
        coff[1:] = np.cumsum(np.repeat(qlen + lengths.astype(np.int64), m))
        dcoff = dev(coff)
        dres = torch.zeros(n * m * dt.itemsize, dtype=torch.uint8, device="cuda")
        dcig = torch.zeros(int(coff[-1]), dtype=torch.int32, device="cuda")
        common = (qlen, n, dch.data_ptr(), doff.data_ptr(), dlen.data_ptr(), int(lengths.max()), -11, -1, dres.data_ptr(),
                  dcig.data_ptr(), dcoff.data_ptr())
        kw = dict(expected_scores=dexp.data_ptr(), trace_bytes=tb)
        if hsps:
            kw.update(max_hsps=m, min_score=1)
        if pssm is None:
            f = capi.align_hsps if hsps else capi.align_hits
            call = lambda **more: f(ctx, dq.data_ptr(), *common, **kw, **more)
        else:
            f = capi.align_hsps_pssm if hsps else capi.align_hits_pssm
            call = lambda **more: f(ctx, dp.data_ptr(), dq.data_ptr(), *common, **kw, **more)
        need = call()
        temp = torch.empty(need, dtype=torch.uint8, device="cuda")
        ms = []
        for rep in range(reps + 1):          # the first call is the warm-up
            start.record()
            call(temp=temp.data_ptr(), temp_bytes=need)
            stop.record()
            torch.cuda.synchronize()
            if rep:
                ms.append(start.elapsed_time(stop))
        res = np.frombuffer(dres.cpu().numpy().tobytes(), dtype=dt)
        assert (res["status"][::m] == capi.ALIGN_OK).all(), res["status"]
        out = spread(ms)
        out["ok_slots"] = int((res["status"] == capi.ALIGN_OK).sum())
        return out

    out = {"align_hits": timed(1, False)}
    if not plain_only:
        out["max_hsps"] = {str(m): timed(m, True) for m in HSPS}
        t = {m: out["max_hsps"][str(m)]["median_ms"] for m in HSPS}
        rounds = {"1": t[2] - t[1], "2-3": (t[4] - t[2]) / 2, "4-7": (t[8] - t[4]) / 4}
        out["vetoed_round_ms"] = {k: round(v, 4) for k, v in rounds.items()}
        out["vetoed_round_over_round0"] = {k: round(v / t[1], 3) for k, v in rounds.items()}
        out["max_hsps_1_over_align_hits"] = round(t[1] / out["align_hits"]["median_ms"], 4)
    return out


def main():
    from cudasw4_amd import synthdb
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=synthdb.SPROT_SEQUENCES)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pssm", action="store_true", help="the PSSM form (from_sequence PSSMs of the same queries)")
    ap.add_argument("--plain-only", action="store_true", help="time sw_align_hits only")
    args = ap.parse_args()
    import torch
    from cudasw4_amd import capi, driver, pssm
    table = driver.matrix(62)
    chars, offsets, lengths = synthdb.sprot_like(args.n)
    _, letters = driver.read_sequences(os.path.join(ROOT, "tests", "golden", "allqueries.fasta"))
    d = driver.Driver(devices=[0], num_top=100, kinds=(0, 0, 3, 3))
    d.db_from_arrays(chars, offsets, lengths)
    d.upload()
    ctx = capi.Context(0)
    ctx.set_matrix(table)
    subject = lambda i: chars[int(offsets[i]):int(offsets[i]) + int(lengths[i])]
    out = {"metric": "align_hsps_pssm" if args.pssm else "align_hsps", "library": os.path.relpath(capi.LIB_PATH, ROOT),
           "db_sequences": int(len(lengths)), "reps": args.reps, "min_score": 1, "queries": []}
    for q_letters in letters:
        if len(q_letters) not in (144, 464, 1000):
            continue
        q = driver.encode(q_letters)
        r = d.scan(q_letters)
        entry = {"qlen": len(q)}
        for top in (10, 100):
            ids, scores = r["ids"][:top], r["scores"][:top]
            entry["top%d" % top] = time_calls(torch, capi, ctx, q, [subject(i) for i in ids], scores, args.reps,
                                              pssm.from_sequence(q, table) if args.pssm else None, args.plain_only)
        out["queries"].append(entry)
    d.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
