#!/usr/bin/env python3
"""Cost of masking the subjects on the GPU on the Swiss-Prot-like synthetic DB: HIP-event times of
sw_mask_subjects over the whole DB (out of place, so that every repetition does the same work) as a whole and per launch,
the host-to-device copy of the same bytes from pinned memory, and the scans of the 144- and 1000-residue golden queries
through the host driver — resident, and under a memory limit that streams the whole DB on every query (`--stream-mem`, with
hybrid residency off so that nothing stays cached) — with masking on and off in the same session.  Medians of `--reps` after a warm-up.  Prints one JSON line.

    python tools/mask_bench.py [--n 570000] [--reps 5] [--stream-mem 419430400] [--batch-bytes 33554432]
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
    ap.add_argument("--stream-mem", type=int, default=400 << 20, help="--maxGpuMem of the streamed scans (the staging buffers are cut from it)")
    ap.add_argument("--batch-bytes", type=int, default=32 << 20)
    ap.add_argument("--window", type=int, default=12)
    ap.add_argument("--trigger", type=float, default=1.9)
    ap.add_argument("--extend", type=float, default=2.2)
    args = ap.parse_args()
    import torch
    from cudasw4_amd import capi, driver, mask
    assert torch.cuda.is_available(), "mask_bench needs a GPU"
    chars, offsets, lengths = synthdb.sprot_like(args.n)
    chars = np.ascontiguousarray(chars, dtype=np.int8)
    n, nbytes, residues = len(lengths), int(offsets[-1]), int(np.asarray(lengths).astype(np.int64).sum())
    params = (args.window, mask.threshold(args.window, args.trigger), mask.threshold(args.window, args.extend))

    # ---- the kernels alone
    ctx = capi.Context(0)
    host = torch.from_numpy(chars.view(np.uint8)).pin_memory()
    dc = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    do = torch.from_numpy(np.asarray(offsets).astype(np.int64)).cuda()
    dl = torch.from_numpy(np.ascontiguousarray(lengths, dtype=np.int32)).cuda()
    out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    need = capi.mask_subjects_temp_bytes(ctx, do.data_ptr(), n, *params)
    temp = torch.empty(need // 8 + 1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    upload_ms, whole_ms, phase_ms, inplace_ms = [], [], [], []
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for e in evs:
        e.record()
    torch.cuda.synchronize()
    handles = [int(e.cuda_event) for e in evs]
    for rep in range(args.reps + 1):
        e0.record()
        dc.copy_(host, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        up = e0.elapsed_time(e1)
        cnt.zero_()
        e0.record()
        capi.mask_subjects(ctx, dc.data_ptr(), do.data_ptr(), dl.data_ptr(), n, *params, out=out.data_ptr(), temp=temp.data_ptr(),
                           temp_bytes=need, counts=cnt.data_ptr(), stream=stream)
        e1.record()
        torch.cuda.synchronize()
        whole = e0.elapsed_time(e1)
        counts = cnt.cpu().tolist()
        capi.mask_subjects_phases(ctx, dc.data_ptr(), do.data_ptr(), dl.data_ptr(), n, *params, out=out.data_ptr(), temp=temp.data_ptr(),
                                  temp_bytes=need, events=handles, stream=stream)
        torch.cuda.synchronize()
        phases = [evs[i].elapsed_time(evs[i + 1]) for i in range(3)]
        e0.record()   # in place, on the fresh copy: what the driver does behind an upload
        capi.mask_subjects(ctx, dc.data_ptr(), do.data_ptr(), dl.data_ptr(), n, *params, out=dc.data_ptr(), temp=temp.data_ptr(),
                           temp_bytes=need, stream=stream)
        e1.record()
        torch.cuda.synchronize()
        if rep:
            upload_ms.append(up)
            whole_ms.append(whole)
            phase_ms.append(phases)
            inplace_ms.append(e0.elapsed_time(e1))
    assert bool((out == dc).all()), "in place and out of place disagree"
    del host, dc, out, temp
    ctx.close()
    torch.cuda.empty_cache()

    # ---- the driver: the same two queries, resident and streamed, masking off and on
    _, letters = driver.read_sequences(os.path.join(ROOT, "tests", "golden", "allqueries.fasta"))
    queries = {ql: [x for x in letters if len(x) == ql][0] for ql in (144, 1000)}
    scans = {}
    for mode, kw in (("resident", {}), ("streamed", dict(max_gpu_mem=args.stream_mem, max_batch_bytes=args.batch_bytes))):
        os.environ["CUDASW4_AMD_NO_HYBRID"] = "1" if mode == "streamed" else "0"
        for masking in (False, True):
            d = driver.Driver(devices=[0], num_top=10, **kw)
            if masking:
                d.set_subject_masking(True, args.window, args.trigger, args.extend)
            d.db_from_arrays(chars, offsets, lengths)
            d.upload()
            for ql, q in queries.items():
                ms = [d.scan(q)["seconds"] * 1e3 for _ in range(args.reps + 1)][1:]
                scans["%s_%d_%s" % (mode, ql, "masked" if masking else "plain")] = {"ms": round(float(np.median(ms)), 3),
                                                                                   "all": [round(x, 3) for x in ms]}
            if masking:
                c = d.masking_counts()
                assert [c["positions"], c["subjects"]] == counts and c["residues_seen"] == residues, (c, counts)
            if mode == "streamed":
                info = d.shard_info(0)
                assert not info["resident"] and info["cached_chars"] == 0, info
                scans["streamed_batches"] = len(d.batch_intervals())
            d.close()
    med = lambda v: round(float(np.median(v)), 4)
    ph = np.median(np.array(phase_ms), axis=0)
    launches = float(ph.sum())
    line = {"metric": "mask_bench", "db_sequences": n, "db_bytes": nbytes, "db_residues": residues, "reps": args.reps,
            "window": params[0], "trigger_sum": params[1], "extend_sum": params[2],
            "masked_positions": counts[0], "masked_subjects": counts[1], "masked_fraction": round(counts[0] / residues, 6),
            "mask_call_ms": med(whole_ms), "mask_call_ms_all": [round(x, 4) for x in whole_ms],
            "mask_in_place_ms": med(inplace_ms),
            "flags_ms": round(float(ph[0]), 4), "resolve_ms": round(float(ph[1]), 4), "apply_ms": round(float(ph[2]), 4),
            "launches_ms": round(launches, 4), "mask_gresidues_per_s": round(residues / launches / 1e6, 2),
            "upload_ms": med(upload_ms), "upload_gb_per_s": round(nbytes / med(upload_ms) / 1e6, 2),
            "mask_over_upload": round(launches / med(upload_ms), 4), "scratch_bytes": need, "scans": scans}
    for ql in (144, 1000):
        a, b = scans["streamed_%d_plain" % ql]["ms"], scans["streamed_%d_masked" % ql]["ms"]
        line["streamed_%d_masking_costs_ms" % ql] = round(b - a, 3)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
