#!/usr/bin/env python3
"""MSA selection timing (sw_msa_select): HIP-event times of its three stages (rows, levels, select) for the top-500 and the
top-16384 hits of the 464-residue golden query on the Swiss-Prot-like synthetic DB — the configuration of tools/msa_bench.py —
next to sw_msa_filter on the same hits in the same run (its three stages), to sw_align_hits of those hits, and to the numpy
restatement (cudasw4_amd.msa.select_rows) on the same rows.  Medians of --reps runs after one warm-up pass.  Prints one JSON
line.

    python tools/msa_select_bench.py [--n 570000] [--tops 500,16384] [--reps 5] [--diff 1000] [--identity 90] [--host-rows 2048]

select_rows makes one pass over all rows per kept row, so its time grows with kept rows x rows x qlen: above --host-rows rows
it is timed on the first --host-rows rows and scaled by (kept x rows) of the device's result over (kept x rows) of the timed
part (the line says which: host_rows_timed)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from msa_bench import dbdata  # noqa: E402


def one_top(torch, capi, msa, ctx, q, chars, offsets, lengths, result, reps, diff, ladder, host_rows):
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
    dstate = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
    dcounts = torch.zeros(4, dtype=torch.int32, device="cuda")
    ddepth = torch.zeros(qlen, dtype=torch.int32, device="cuda")
    hits = (dq.data_ptr(), qlen, n, dch.data_ptr(), doff.data_ptr(), dlen.data_ptr(), dres.data_ptr(), dcig.data_ptr(), 0)
    filt = lambda **kw: capi.msa_filter(ctx, *hits, ladder[-1], dresid.data_ptr(), dkeep.data_ptr(), dpurged.data_ptr(), **kw)
    sel = lambda **kw: capi.msa_select(ctx, *hits, 0, 0, diff, ladder, dstate.data_ptr(), dresid.data_ptr(), dcounts.data_ptr(),
                                       depth=ddepth.data_ptr(), rows=drows.data_ptr(), **kw)
    fneed, sneed = filt(), sel()
    ftemp = torch.empty(fneed, dtype=torch.uint8, device="cuda")
    stemp = torch.empty(sneed, dtype=torch.uint8, device="cuda")
    aev, fev, sev = ([torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(3))
    for e in aev + fev + sev:
        e.record()
    torch.cuda.synchronize()
    handles = lambda evs: [int(e.cuda_event) for e in evs]
    align_ms, filt_ms, sel_ms = [], [], []
    for _ in range(reps + 1):   # (the first pass warms up and is dropped)
        align(temp=temp.data_ptr(), temp_bytes=need, phase_events=handles(aev))
        filt(temp=ftemp.data_ptr(), temp_bytes=fneed, phase_events=handles(fev))
        sel(temp=stemp.data_ptr(), temp_bytes=sneed, phase_events=handles(sev))
        torch.cuda.synchronize()
        align_ms.append(aev[0].elapsed_time(aev[3]))
        filt_ms.append([fev[i].elapsed_time(fev[i + 1]) for i in range(3)])
        sel_ms.append([sev[i].elapsed_time(sev[i + 1]) for i in range(3)])
    align_ms = float(np.median(align_ms[1:]))
    filt_ms = np.median(np.array(filt_ms[1:]), axis=0).tolist()
    sel_ms = np.median(np.array(sel_ms[1:]), axis=0).tolist()
    rows = drows.cpu().numpy().reshape(n + 1, qlen)
    state, counts = dstate.cpu().numpy(), dcounts.cpu().numpy().tolist()
    depth = ddepth.cpu().numpy()
    # at full size, two checks that need no host selection: the depth is the column sum of the kept rows, and with D = 0 and
    # the one rung the states are sw_msa_filter's keep
    assert depth.tolist() == (rows[state == 1] < 20).sum(axis=0).tolist()
    capi.msa_select(ctx, *hits, 0, 0, 0, ladder[-1:], dstate.data_ptr(), dresid.data_ptr(), dcounts.data_ptr(), temp=stemp.data_ptr(),
                    temp_bytes=sneed)
    torch.cuda.synchronize()
    keep = dkeep.cpu().numpy()
    assert (dstate.cpu().numpy() == 1).astype(int).tolist() == keep.tolist() and int(dcounts[3].item()) == int(dpurged.item())
    # the host restatement on the same rows (the master last, as the module wants it)
    m = min(n, host_rows)
    part = np.concatenate([rows[:m], rows[n:]])
    t0 = time.perf_counter()
    hstate, hdepth, hcounts = msa.select_rows(part, 0, 0, diff, ladder)
    host_s = time.perf_counter() - t0
    if m == n:
        assert hstate.tolist() == state.tolist() and hcounts == counts and hdepth.tolist() == depth.tolist()
    work = lambda kept, k: max((kept + 1) * (k + 1), 1)
    host_full_s = host_s * work(counts[0], n) / work(hcounts[0], m)
    r4 = lambda v: round(v, 4)
    return {"hits": n, "temp_bytes": sneed, "kept": counts[0], "thinned": counts[3], "filter_kept": int(keep[:n].sum()),
            "rows_ms": r4(sel_ms[0]), "levels_ms": r4(sel_ms[1]), "select_ms": r4(sel_ms[2]), "total_ms": r4(sum(sel_ms)),
            "filter_rows_ms": r4(filt_ms[0]), "filter_pairs_ms": r4(filt_ms[1]), "filter_greedy_ms": r4(filt_ms[2]),
            "filter_total_ms": r4(sum(filt_ms)), "align_hits_ms": r4(align_ms), "select_over_align": round(sum(sel_ms) / align_ms, 5),
            "levels_over_filter_pairs": round(sel_ms[1] / max(filt_ms[1], 1e-9), 3),
            "host_rows_timed": m, "host_kept_timed": hcounts[0], "host_select_s_timed": r4(host_s), "host_select_s": round(host_full_s, 3),
            "host_over_device": round(host_full_s * 1e3 / sum(sel_ms), 1)}


def main():
    from cudasw4_amd import synthdb
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=synthdb.SPROT_SEQUENCES)
    ap.add_argument("--tops", default="500,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--qlen", type=int, default=464)
    ap.add_argument("--diff", type=int, default=1000)
    ap.add_argument("--identity", type=int, default=90)
    ap.add_argument("--host-rows", type=int, default=2048)
    args = ap.parse_args()
    import torch
    from cudasw4_amd import capi, driver, msa
    ladder = msa.default_ladder(args.identity)
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
    out = {"metric": "msa_select", "db_sequences": int(len(lengths)), "qlen": len(q), "reps": args.reps, "diff": args.diff,
           "ladder": ladder}
    for top in tops:
        result = {"ids": full["ids"][:top], "scores": full["scores"][:top]}
        out["top%d" % top] = one_top(torch, capi, msa, ctx, q, chars, offsets, lengths, result, args.reps, args.diff, ladder,
                                     args.host_rows)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
