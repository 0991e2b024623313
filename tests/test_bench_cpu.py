"""CPU: bench.py's launcher logic, the one launch planner / shard cutter shared by the C++ driver and the Python
mirror, and the synthetic DB generator.  No GPU, no compute calls."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np

import oracle_lib as O

ROOT = O.ROOT


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_bench_spawn_command_and_defaults():
    b = load_bench()
    a = b.parse_args(["--gpus", "8", "--steps", "3", "--warmup", "1"])
    assert a.gpus == 8 and a.scaling == "strong" and a.workload == "peak" and a.top == 10
    cmd = b.spawn_command(8, ["--gpus", "8", "--steps", "3"], 29511)
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "8"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-4:] == ["--gpus", "8", "--steps", "3"]
    assert b.kinds_for(b.parse_args([]))[1] == (0, 0, 3, 3)
    assert b.kinds_for(b.parse_args(["--workload", "sprot-like"]))[1] == (1, 1, 2, 2)
    assert b.kinds_for(b.parse_args(["--kernel", "dpxs32"]))[1] == (2, 1, 2, 2)
    assert b.parse_size("1G") == 1 << 30 and b.parse_size("0") == 0


def test_bench_plain_run_and_full_switch():
    """Without --full a run is the headline alone (every extra leg off); --full leaves the --no-* switches to the caller;
    --steps is the number of timed steps and must be at least 1."""
    b = load_bench()
    plain = b.parse_args(["--steps", "7", "--warmup", "2"])
    assert not plain.full and plain.steps == 7 and plain.warmup == 2 and plain.dump_outputs is None
    assert plain.no_cpu_baseline and plain.no_verify and plain.no_secondary and plain.no_sweep and plain.no_shard_proxy
    full = b.parse_args(["--full", "--no-sweep", "--dump-outputs", "out"])
    assert full.full and full.no_sweep and full.dump_outputs == "out"
    assert not (full.no_cpu_baseline or full.no_verify or full.no_secondary or full.no_shard_proxy)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert p.returncode == 2 and "--steps" in p.stderr


def test_bench_dump_outputs_writes_the_last_steps_lists(tmp_path):
    """--dump-outputs: per query the merged top-K scores / ids (-1 past a short list) and the overflow counts, float64;
    a top-K too large for the 64 MB budget is written as a fixed, seeded sample of its columns."""
    b = load_bench()
    results = [{"num_overflows": 1, "num_rescored": 2}, {"num_overflows": 0, "num_rescored": 0}]
    merged = [(np.array([50, 40, 30], np.int32), np.array([7, 3, 9])), (np.array([20], np.int32), np.array([4]))]
    b.dump_outputs(str(tmp_path / "d"), results, merged, 3)
    got = {n: np.load(str(tmp_path / "d" / (n + ".npy"))) for n in ("top_scores", "top_ids", "num_overflows", "num_rescored")}
    assert all(v.dtype == np.float64 for v in got.values())
    assert got["top_scores"].tolist() == [[50, 40, 30], [20, -1, -1]] and got["top_ids"].tolist() == [[7, 3, 9], [4, -1, -1]]
    assert got["num_overflows"].tolist() == [1, 0] and got["num_rescored"].tolist() == [2, 0]
    K = 3_000_000
    big = [(np.arange(K, 0, -1, dtype=np.int32), np.arange(K))] * 2
    for d in ("e", "f"):
        b.dump_outputs(str(tmp_path / d), results, big, K)
    total = sum(os.path.getsize(str(tmp_path / "e" / f)) for f in os.listdir(str(tmp_path / "e")))
    assert total <= 64 << 20
    e, f = np.load(str(tmp_path / "e" / "top_ids.npy")), np.load(str(tmp_path / "f" / "top_ids.npy"))
    assert e.shape[1] < K and np.array_equal(e, f) and (np.diff(e[0]) > 0).all()


def test_roofline_arithmetic_uses_the_device_and_the_measured_peaks():
    """the VALU peak comes from the device's own CU count, the in-process micro-run and the sampled clock;
    nothing is hard-coded but the nominal clock, which is named."""
    b = load_bench()
    cal = {"cus": 304, "mix": {"0": {"lane_instr_per_s": 3.6e13}, "1": {"lane_instr_per_s": 6.0e13}, "2": {"lane_instr_per_s": 4.4e13},
                               "3": {"lane_instr_per_s": 3.7e13}, "4": {"lane_instr_per_s": 4.0e13}}}
    sclk = {"avg_mhz": 2100.0}
    nominal, measured, at_clock, lanes, cus = b.valu_peaks(0, cal, sclk)
    # packed kinds are priced against the micro-run of the kernels' OWN mix with conflict-free operands (4), not the pure VOP3P
    # stream (0): VERDICT r5 item 5
    assert cus == 304 and lanes == 64.0 and nominal == 304 * 64.0 * 2.4e9 and measured == 4.0e13 and at_clock == 304 * 64.0 * 2.1e9
    assert b.valu_peaks(3, cal, None)[1:3] == (6.0e13, None) and b.valu_peaks(2, cal, sclk)[1] == 4.4e13
    assert b.valu_peaks(1, None, None)[:2] == (256 * 64.0 * 2.4e9, None)       # no calibration: the planning figures, and no measured peak
    # the CPU team rule: the best sustained rate (ties within 2 %: the smaller team)
    assert b.pick_team({128: 9.1, 64: 10.0, 32: 9.9, 16: 8.0}) == 32
    assert b.pick_team({128: 5.0, 64: 10.0, 32: 9.5, 16: 8.0}) == 64
    events = [{"eff_kind": 0, "rows": 32, "lanes": 16, "nstripes": 2, "ms": 100.0, "chars": 5.12e8, "cells": 5.12e11, "subjects": 10 ** 6,
               "qlen": 1000, "t0_ms": 0.0, "t1_ms": 100.0}]

    class A:
        steps = 1
    roof, valu, table = b.roofline_objects(A(), "peak", "half2", events, {"resident": True}, cal, sclk)
    assert roof["peak"] == 8000.0 and 0 < roof["frac"] < 0.01 and valu["cus"] == 304 and valu["peak_measured"] == 40.0
    assert valu["kernel_gcups"] == 5120.0 and valu["observed_sclk"] == sclk and valu["peak_at_observed_clock"] == round(304 * 64 * 2.1e9 / 1e12, 3)
    if valu["frac"] is not None:
        assert abs(valu["frac_of_measured_peak"] * 4.0e13 - valu["frac"] * 304 * 64.0 * 2.4e9) < 6e9   # (both fractions are rounded to four digits)
        assert abs(valu["frac_of_128"] * 2 - valu["frac"]) < 2e-4      # the same achieved rate against 128 lanes/clk/CU


def test_cpu_baseline_calibration_and_sampling_arithmetic():
    """the team sweep measures what the legs measure — the whole query set, sustained — and the ragged
    leg's timed sample is a uniform draw without the giants (checked apart)."""
    b = load_bench()
    queries = [np.zeros(n, np.int8) for n in (100, 300, 600)]
    lengths = np.full(40000, 64, np.int32)
    offsets = np.arange(40001, dtype=np.uint64) * 64
    chars = np.zeros(40000 * 64, np.int8)
    calls = []
    clock = [0.0]
    rate_of = {8: 8e9, 4: 4e9, 2: 2e9, 1: 0.5e9}   # cells per second a team sustains

    def fake_scan(q, c, o, l, nt):
        calls.append((len(q), len(l), nt))
        clock[0] += len(q) * float(l.sum()) / rate_of[nt]
    real = b.time.perf_counter
    b.time.perf_counter = lambda: clock[0]
    try:
        sweep = b.calibrate_team(queries, chars, offsets, lengths, fake_scan, 8, min_seconds=0.5)
    finally:
        b.time.perf_counter = real
    assert sorted(sweep) == [1, 2, 4, 8]
    for nt, r in sweep.items():   # the rate of the whole set, warm-up call excluded ... close to what the fake sustains
        assert abs(r - rate_of[nt] / 1e9) / (rate_of[nt] / 1e9) < 0.35, (nt, r)
    # every team ran ALL queries, on a slice in proportion to the team (3 blocks of 32 subjects per thread)
    for nt in (1, 2, 4, 8):
        mine = [c for c in calls if c[2] == nt]
        assert {c[0] for c in mine[1:]} == {100, 300, 600} and {c[1] for c in mine} == {nt * 3 * 32}
    assert b.pick_team(sweep) == 8
    c, o, l = b.calibration_sample(chars, offsets, lengths, 128)
    assert len(l) == 128 * 3 * 32 and len(o) == len(l) + 1 and len(c) == len(l) * 64
    assert len(b.calibration_sample(chars, offsets, lengths[:100], 128)[2]) == 100     # never more than the sample holds
    pick, giants = b.cpu_sample_of(570000, 20000)
    assert giants.tolist() == [569996, 569997, 569998, 569999] and len(np.intersect1d(pick, giants)) == 0
    assert 19990 <= len(pick) <= 20000 and (np.diff(pick) > 0).all()
    assert abs(pick.mean() / 570000 - 0.5) < 0.01     # uniform over the length-sorted DB
    ncpu, quota = b.cpu_quota()
    assert ncpu >= 1 and (quota is None or quota > 0)


def test_bench_refuses_mismatched_world_size():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True, text=True, env=env)
    assert p.returncode == 2 and "WORLD_SIZE" in p.stderr


def test_bench_counters_are_tied_to_the_kernel_sources():
    b = load_bench()
    c, note = b.load_counters()
    assert (c is None) != (note is None)
    if c is not None:
        assert c["kernel_src_sha16"] == b.kernel_source_sha()


def reference_walk(lengths, kinds):
    """The partition walk restated independently (cudasw4.cuh:1742-2103 + merging of equal kinds): partition 35 always
    alone; partition 34 alone while it holds fewer than 512 subjects (wave-wide groups), else part of the bulk."""
    bounds = O.partition_boundaries()
    ends = np.searchsorted(lengths, bounds, side="right")
    begins = np.concatenate([[0], ends[:-1]])
    runs, last_bulk = [], False
    for p in range(35, -1, -1):
        b, e = int(begins[p]), int(ends[p])
        if e <= b:
            continue
        kind = kinds[0] if p < 34 else kinds[1] if p == 34 else kinds[2]
        bulk = p < 34 or (p == 34 and e - b >= 512)
        if runs and runs[-1]["kind"] == kind and runs[-1]["begin"] == e and bulk and last_bulk:
            runs[-1]["begin"] = b
        else:
            runs.append({"kind": kind, "part_id": 33 if (p == 34 and bulk) else p, "begin": b, "end": e, "maxlen": int(lengths[e - 1])})
        last_bulk = bulk
    return runs


def test_one_planner_for_both_host_drivers():
    from cudasw4_amd import driver, search
    rng = np.random.default_rng(0)
    merged = 0
    for trial in range(24):
        n = int(rng.integers(1, 400)) if trial < 16 else int(rng.integers(3000, 9000))
        lengths = np.sort(rng.choice([3, 48, 49, 64, 65, 200, 256, 257, 512, 700, 1280, 1281, 5000, 8000, 8001, 20000], n)).astype(np.int32)
        for kinds in ((0, 0, 3), (1, 1, 2), (2, 1, 2), (3, 0, 3)):
            got = driver.plan_runs(lengths, *kinds)
            assert got == reference_walk(lengths, kinds), (trial, kinds)
            merged += any(r["part_id"] == 33 and r["maxlen"] > 1280 for r in got)
    assert merged > 0  # partition 34 joined the bulk launch somewhere
    # a large partition 34 of the bulk's kind: ONE bulk run + the giants
    lengths = np.sort(np.concatenate([np.full(5000, 300), np.full(600, 2000), np.full(3, 9000)])).astype(np.int32)
    got = driver.plan_runs(lengths, 1, 1, 2)
    assert [(r["part_id"], r["begin"], r["end"], r["maxlen"]) for r in got] == [(35, 5600, 5603, 9000), (33, 0, 5600, 2000)]
    # other kind for partition 34: a run of its own on the bulk shape (reported as 33); a small one: wave-wide groups (34)
    assert [r["part_id"] for r in driver.plan_runs(lengths, 2, 1, 2)] == [35, 33, 15]
    assert [r["part_id"] for r in driver.plan_runs(lengths[:5100], 1, 1, 2)] == [34, 15]
    assert driver.plan_runs(np.zeros(0, np.int32), 0, 0, 3) == []
    # latency mode (small shards of real DBs): partition 34 keeps a launch of its own whatever its size — three runs, the
    # same subjects, every subject in exactly one of them
    lat = driver.plan_runs(lengths, 1, 1, 2, latency_mode=True)
    assert [(r["part_id"], r["begin"], r["end"], r["maxlen"]) for r in lat] == [(35, 5600, 5603, 9000), (34, 5000, 5600, 2000), (15, 0, 5000, 300)]
    for trial in range(8):
        ls = np.sort(rng.choice([3, 64, 700, 1280, 1281, 5000, 8000, 8001, 20000], int(rng.integers(600, 5000)))).astype(np.int32)
        runs = driver.plan_runs(ls, 1, 1, 2, latency_mode=True)
        covered = sorted((r["begin"], r["end"]) for r in runs)
        assert covered[0][0] == 0 and covered[-1][1] == len(ls) and all(a[1] == b[0] for a, b in zip(covered, covered[1:]))
        assert all(r["part_id"] >= 34 or r["maxlen"] <= 1280 for r in runs)       # nothing of partition 34 inside a bulk run
    # the Python mirror's merged plan IS the C++ planner's
    import inspect
    assert "driver.plan_runs" in inspect.getsource(search.Searcher._launch_plan)


def test_shard_ranges_cover_and_balance():
    from cudasw4_amd import driver, synthdb
    lengths = synthdb.sprot_like_lengths(20000, seed=1, max_len=9000)
    chars, offsets, lengths = synthdb.random_db(lengths, seed=2)
    for world in (1, 2, 3, 8):
        r = driver.shard_ranges(offsets, lengths, world)
        assert len(r) == world and all(len(x) == 36 for x in r)
        covered = np.zeros(len(lengths), dtype=np.int32)
        per_rank_chars = []
        for rank in range(world):
            c = 0
            for (b, e) in r[rank]:
                covered[b:e] += 1
                c += int(offsets[e] - offsets[b])
            per_rank_chars.append(c)
        assert (covered == 1).all()
        if world > 1:
            assert max(per_rank_chars) < 1.25 * (sum(per_rank_chars) / world)


def test_synthetic_sprot_like_db_layout():
    from cudasw4_amd import synthdb
    l = synthdb.sprot_like_lengths(30000)
    assert (np.diff(l) >= 0).all() and l[0] >= 2 and l[-1] == synthdb.SPROT_MAX_LENGTH
    chars, offsets, lengths = synthdb.random_db(l[:3000], seed=9, other_fraction=0.05)
    assert offsets[0] == 0 and len(offsets) == 3001 and (np.diff(offsets.astype(np.int64)) == (lengths.astype(np.int64) + 3) // 4 * 4).all()
    for i in (0, 17, 2999):
        s = chars[int(offsets[i]):int(offsets[i + 1])]
        assert (s[lengths[i]:] == 20).all() and s[:lengths[i]].max() <= 20 and s.min() >= 0
    a = synthdb.sprot_like(2000)
    b = synthdb.sprot_like(2000)
    assert all((x == y).all() for x, y in zip(a, b))


def test_sprot_like_db_carries_families_of_the_queries():
    """The Swiss-Prot stand-in holds what a real Swiss-Prot holds for these queries: the proteins
    themselves and seeded relatives — so scans see hits far above the noise floor, packed overflows and re-scores —
    while sequence count, length histogram, sort order and layout stay those of the background."""
    from cudasw4_amd import synthdb
    n = 40000
    chars, offsets, lengths, fam = synthdb.sprot_like(n, return_family_ids=True)
    plain = synthdb.sprot_like(n, families=False)
    assert (lengths == plain[2]).all() and (offsets == plain[1]).all() and len(chars) == len(plain[0])
    assert (np.diff(lengths) >= 0).all() and chars.min() >= 0 and chars.max() <= 20
    ends = offsets[:-1].astype(np.int64) + lengths
    assert all((chars[int(e):int(o)] == 20).all() for e, o in list(zip(ends, offsets[1:]))[::997])
    assert 100 < len(fam) < n // 20 and (np.diff(fam) > 0).all()
    # only family slots differ from the background
    changed = np.nonzero([not np.array_equal(chars[int(offsets[i]):int(offsets[i + 1])], plain[0][int(offsets[i]):int(offsets[i + 1])])
                          for i in fam])[0]
    assert len(changed) == len(fam)
    untouched = np.setdiff1d(np.arange(0, n, 53), fam)
    assert all(np.array_equal(chars[int(offsets[i]):int(offsets[i + 1])], plain[0][int(offsets[i]):int(offsets[i + 1])]) for i in untouched)
    # composition of the background: Swiss-Prot's, not uniform
    freq = np.bincount(plain[0][plain[0] < 20], minlength=20) / float((plain[0] < 20).sum())
    assert abs(freq[10] - 0.0965) < 0.003 and abs(freq[17] - 0.011) < 0.002     # L and W
    # the queries find themselves (self score, Appendix B of SURVEY.md) and relatives above the packed limits
    _, qs = O.load_queries()
    from cudasw4_amd import search
    sub = search.build_shard(chars, offsets, lengths, [(int(i), int(i) + 1) for i in fam])[:3]
    golden = json.load(open(os.path.join(O.GOLDEN_DIR, "ref_scores.json")))
    self_scores = [golden["allvsall"][i][i] for i in range(20)] if "allvsall" in golden else None
    over_f16 = 0
    for qi in (4, 9, 16):
        sc = O.scan(qs[qi], *sub, simd=True)
        if self_scores:
            assert int(sc.max()) == self_scores[qi]
        over_f16 += int((sc >= 2048).sum())
        assert (sc >= 1000).sum() >= (2 if qi < 10 else 1)   # long proteins are rare: a long query may only find itself
    assert over_f16 >= 10
    q16 = O.scan(qs[16], *sub, simd=True)
    assert int(q16.max()) >= 25000                                              # an int16 overflow as well
    # small DBs get proportionally small families, and the generator is deterministic
    small = synthdb.sprot_like(2000, return_family_ids=True)
    assert 20 <= len(small[3]) <= 200
    assert all((x == y).all() for x, y in zip(synthdb.sprot_like(n, return_family_ids=True), (chars, offsets, lengths, fam)))


def test_union_of_launch_intervals():
    b = load_bench()
    assert b.union_ms([]) == 0.0
    assert b.union_ms([(0.0, 2.0), (1.0, 3.0), (5.0, 6.0)]) == 4.0          # overlap counted once, gap not at all
    assert b.union_ms([(5.0, 6.0), (0.0, 10.0)]) == 10.0                    # a launch inside another
    assert b.union_ms([(0.0, 1.0), (1.0, 2.0), (2.0, 3.0)]) == 3.0          # a sequence of batches adds up


def fake_event(kind, rows, lanes, nstripes, t0, t1, chars, qlen=512, eff=None):
    n = chars // 512
    return {"gpu": 0, "kind": kind, "part_id": 21, "qlen": qlen, "subjects": n, "cells": float(qlen) * chars, "chars": float(chars),
            "ms": t1 - t0, "t0_ms": t0, "t1_ms": t1, "eff_kind": kind if eff is None else eff, "rows": rows, "nstripes": nstripes,
            "lanes": lanes}


def test_roofline_accounting_of_sequential_and_overlapping_launches(monkeypatch):
    """A streamed scan is a SEQUENCE of batch launches (round 2 counted it with its longest launch and reported a VALU
    fraction of 2.457); launches on different streams overlap.  The kernels' own rate is cells / the union of the
    intervals, the HBM traffic of a launch scales with its subject bytes, and no fraction can exceed 1 by construction
    when the per-cell instruction count is the measured one."""
    b = load_bench()
    args = b.parse_args(["--steps", "1"])
    counters = {"kernel_src_sha16": "x",
                "valu_instr_per_unit": {"peak:half2:resident": {"value": 6.3, "source": "profiles/fake_pmc.txt"}},
                "traffic_bytes_per_char": {"peak|sw_scan_kernel<0, 43, 16, true,": {"value": 60.0, "nstripes": [8], "source": "profiles/fake_pmc.txt"}}}
    monkeypatch.setattr(b, "load_counters", lambda: (counters, None))
    # four 128 MB batches one after the other, 64 ms each, at the rate of a VALU-bound kernel (~11.5 TCUPS at qlen 5478)
    batch = 128 << 20
    ev = [fake_event(0, 43, 16, 8, 64.0 * i, 64.0 * (i + 1), batch, qlen=5478) for i in range(4)]
    # a long-subject launch on an auxiliary stream next to the first batch: overlaps, adds cells but no busy time
    ev.append(fake_event(3, 8, 64, 11, 0.0, 40.0, 1 << 20, qlen=5478))
    roof, valu, table = b.roofline_objects(args, "peak", "half2", ev, {"resident": False, "cached_chars": 0, "chars": 4 * batch})
    assert valu["kernel_busy_ms_per_step"] == 256.0
    cells = sum(e["cells"] for e in ev)
    assert abs(valu["kernel_gcups"] - cells / 1e9 / 0.256) < 1.0
    assert 0 < valu["frac"] <= 1.0 and valu["counters_key"] == "peak:half2:resident"   # falls back to the resident figure
    assert roof["launches"] == 4 and roof["kernel"].startswith("sw_scan_kernel<f16x2, R=43, 16 lanes, multi")
    assert roof["traffic"] == int(60.0 * batch)      # per subject byte x THIS launch's subject bytes
    assert 0 < roof["frac"] < 1e-2
    assert len(table) == 2 and sum(k["launches"] for k in table) == 5
    # other stripes than the counter was measured with: no figure rather than a wrong one
    ev2 = [fake_event(0, 43, 16, 4, 0.0, 10.0, batch, qlen=2700)]
    roof2, _, _ = b.roofline_objects(args, "peak", "half2", ev2, {"resident": True, "cached_chars": batch, "chars": batch})
    assert roof2["traffic"] is None and "no PMC traffic figure" in roof2["traffic_note"]
    # a configuration without a counter entry reports null, never a borrowed number
    _, valu3, _ = b.roofline_objects(args, "peak", "float", ev2, {"resident": True, "cached_chars": batch, "chars": batch})
    assert valu3["frac"] is None and "peak:float:resident" in valu3["counters_note"]


def test_counter_tool_builds_the_entries_bench_reads(tmp_path, monkeypatch):
    """tools/rocprof_summary.py counters (run by tools/collect_profiles.sh on the GPU box) on a hand-made rocprofv3
    database: instructions per cell pair = SQ_INSTS_VALU x 64 / (cells / 2); traffic per subject byte = (2 x FETCH_SIZE +
    WRITE_SIZE) KB / the subject bytes of the line's kernel table; one entry per workload / configuration / residency with
    its own source; the figure of the larger launches is kept when a streamed run of the same kernel comes later; and
    bench.py's lookups find what the tool wrote."""
    import importlib.util
    import json
    import shutil
    import sqlite3
    root = tmp_path / "repo"
    (root / "tools").mkdir(parents=True)
    (root / "profiles").mkdir()
    for rel in ("cudasw4_amd/csrc/sw_dp_kernel.hpp", "cudasw4_amd/csrc/sw_launch.hpp", "cudasw4_amd/csrc/sw_api.hip", "cudasw4_amd/csrc/Makefile"):
        (root / rel).parent.mkdir(parents=True, exist_ok=True)
        shutil.copy(os.path.join(ROOT, rel), root / rel)
    shutil.copy(os.path.join(ROOT, "tools", "rocprof_summary.py"), root / "tools" / "rocprof_summary.py")
    spec = importlib.util.spec_from_file_location("rs", str(root / "tools" / "rocprof_summary.py"))
    rs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rs)

    name = "void swk::sw_scan_kernel<0, 43, 16, true, true>(swk::ScanParams)"

    def mk(path, rows):
        db = sqlite3.connect(str(path))
        db.execute("create table counters_collection(kernel_name text, counter_name text, value real, duration real)")
        db.executemany("insert into counters_collection values (?,?,?,?)", rows)
        db.commit()

    def run(tag, residency, launches, chars_total, fetch_kb, write_kb, insts):
        mk(tmp_path / (tag + "_f.db"), [(name, "FETCH_SIZE", fetch_kb / launches, 1.0)] * launches)
        mk(tmp_path / (tag + "_w.db"), [(name, "WRITE_SIZE", write_kb / launches, 1.0)] * launches)
        mk(tmp_path / (tag + "_v.db"), [(name, "SQ_INSTS_VALU", insts / launches, 1.0)] * launches)
        line = {"dtype": "f16x2", "config": {"workload": "peak: allqueries.fasta (20 queries, 41752 residues) vs x", "kernel": "half2", "residency": residency},
                "kernels": [{"kernel": "sw_scan_kernel<0, 43, 16, true, *>", "launches": launches, "total_ms": 1.0, "chars": chars_total,
                             "cells": 5478.0 * chars_total, "nstripes": [8]}]}
        (tmp_path / (tag + ".log")).write_text("noise\n" + json.dumps(line) + "\n")
        import contextlib, io
        with contextlib.redirect_stdout(io.StringIO()):
            rs.counters(str(tmp_path / (tag + ".log")), str(tmp_path / (tag + "_f.db")), str(tmp_path / (tag + "_w.db")),
                        str(tmp_path / (tag + "_v.db")), "profiles/%s_pmc.txt" % tag, "abc1234")

    chars = 512_000_000
    cells = 5478.0 * chars
    run("res", "resident", 1, chars, fetch_kb=7.4e6, write_kb=16.8e6, insts=6.3 * (cells / 2) / 64)
    run("hyb", "hybrid", 4, chars, fetch_kb=7.5e6, write_kb=17.0e6, insts=6.4 * (cells / 2) / 64)
    kc = json.load(open(root / "profiles" / "kernel_counters.json"))
    assert abs(kc["valu_instr_per_unit"]["peak:half2:resident"]["value"] - 6.3) < 1e-3
    assert abs(kc["valu_instr_per_unit"]["peak:half2:hybrid"]["value"] - 6.4) < 1e-3
    assert kc["valu_instr_per_unit"]["peak:half2:hybrid"]["source"] == "profiles/hyb_pmc.txt"
    t = kc["traffic_bytes_per_char"]["peak|sw_scan_kernel<0, 43, 16, true,"]
    assert t["chars_per_launch"] == chars and t["source"] == "profiles/res_pmc.txt" and t["nstripes"] == [8]   # the resident figure stays
    assert abs(t["value"] - (2 * 7.4e6 + 16.8e6) * 1024 / chars) < 1e-3
    # bench.py reads exactly these keys
    b = load_bench()
    monkeypatch.setattr(b, "load_counters", lambda: (kc, None))
    ev = [fake_event(0, 43, 16, 8, 0.0, 250.0, chars, qlen=5478)]
    roof, valu, _ = b.roofline_objects(b.parse_args(["--steps", "1"]), "peak", "half2", ev, {"resident": True, "cached_chars": chars, "chars": chars})
    assert roof["traffic"] == int(t["value"] * chars) and valu["instr_per_cell_pair"] == kc["valu_instr_per_unit"]["peak:half2:resident"]["value"]
    assert 0 < valu["frac"] <= 1
