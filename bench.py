#!/usr/bin/env python3
"""bench.py — the reference's benchmarks (runpeakbenchmark.sh / runsprotbenchmark.sh) on MI355X.

    python bench.py --gpus N --steps K --warmup W [--workload peak|sprot-like] [--scaling strong|weak] [--full]
                    [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

`--gpus N` with N > 1 and no WORLD_SIZE in the environment starts the N ranks itself (a torch.distributed.run child,
before this process touches the GPU); under torchrun the ranks come from the environment and must match --gpus.

Workloads
  peak        BASELINE.json configs[1]: all 20 queries of allqueries.fasta against the simulated equal-length DB
              (`--pseudodb 1000000 512`: one mt19937(42) sequence replicated 10^6 times), half2 kernel (f16x2).
  sprot-like  configs[2] with a synthetic stand-in for uniprot_sprot (no network): 570 000 sequences, log-normal
              lengths with a 35 k-residue tail (cudasw4_amd/synthdb.py, seeded), packed-int16 kernels (--dpx).
Everything runs through the C++ host driver (libcudasw4_host.so == `align`'s SearchDriver) on top of the C ABI;
BLOSUM62, gop -11, gex -1, DB resident in HBM (--uploadFull), top-K inside the timed region.

A STEP is one pass of the whole query set over the DB (20 scans incl. overflow re-score, per-GPU top-K and its copy
to the host, then ONE gather of the per-rank lists and the host-side merge) — the unit the reference's
"Total time ... GCUPS" line is computed over (main.cu:257-260).  GCUPS = sum |q| * sum |s| / 1e9 / s with true
lengths (cudasw4.cuh:2264-2271).

Multi-GPU: `--scaling strong` (default): ONE DB is cut into char-balanced shards per length partition
(partitionDBAmongstGpus, cudasw4.cuh:928-1004), rank r scans shard r; no data-path collective, the per-rank top-K
lists are merged on the host of rank 0.  `--scaling weak`: every rank scans its own --db-size subjects.

A plain run sets up, warms up, times --steps steps and prints the line (`metric`, `value`, `unit`, `higher_is_better`,
`dtype`, `ms_per_step`, ...); `--dump-outputs DIR` writes what the last timed step returned (dump_outputs()).  Everything
else is measured with `--full`:

After the timed region every query is scanned once more and EVERY score is checked (peak: against the reference's
golden scores in tests/golden/ref_scores.json; sprot-like: against the CPU oracle on the cpu_baseline sample, or
packed-vs-int32 equality of all scores when there is no CPU leg) -> "verified".

With N > 1 ranks the --full (strong-scaling) line also carries `"weak_scaling": {...}`: the same benchmark with one full
DB per rank.  The --full (peak) run also measures the sprot-like workload afterwards and reports it as `"sprot_like": {...}` in the
same line (its own timed region, verification, roofline and CPU leg), so that BASELINE config 3 is under the same clock.

Prints ONE JSON line on rank 0 (driver contract); with --full including `roofline` and `cpu_baseline`.
"""
import argparse
import contextlib
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KIND_BY_NAME = {"half2": 0, "dpxs16": 1, "dpxs32": 2, "float": 3}
DTYPE_BY_KIND = {0: "f16x2", 1: "i16x2", 2: "i32", 3: "f32"}
# (the sources of the kernels the PMC constants are about: sw_scan_kernel, the streamed kernels and their launcher; sw_rows_pipeline.hpp — the
# row-parallel kernel of the longest subjects — is not counted by them)
KERNEL_SOURCES = ["cudasw4_amd/csrc/sw_dp_kernel.hpp", "cudasw4_amd/csrc/sw_stream_kernel.hpp", "cudasw4_amd/csrc/sw_launch.hpp", "cudasw4_amd/csrc/sw_api.hip",
                  "cudasw4_amd/csrc/Makefile"]


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", choices=["peak", "sprot-like", "uniref50-like", "trembl-like"], default="peak")
    ap.add_argument("--queries", default=None, help="comma-separated indices into allqueries.fasta (default: all 20)")
    ap.add_argument("--shards-per-gpu", type=int, default=1,
                    help="in-process shards per rank, all on this rank's GPU (one worker thread, context and stream set each): the "
                         "shape of an N-GPU node on one device")
    ap.add_argument("--scaling", choices=["strong", "weak"], default="strong",
                    help="N > 1: shard ONE DB over the ranks (strong, default) or give every rank its own DB (weak)")
    ap.add_argument("--db-size", type=int, default=None, help="subjects of the DB (peak: 1000000, sprot-like: 570000, uniref50-like: 60000000, trembl-like: 250000000)")
    ap.add_argument("--db-length", type=int, default=512, help="peak: pseudo-DB subject length")
    ap.add_argument("--kernel", choices=sorted(KIND_BY_NAME) + ["dpx"], default=None,
                    help="kernel configuration (peak default: half2; sprot-like default: dpx = DPXs16/DPXs16/DPXs32/DPXs32)")
    ap.add_argument("--top", type=int, default=10, help="top-K per query inside the timed region (reference scripts: 0)")
    ap.add_argument("--max-gpu-mem", default="0", help="per-GPU memory limit (K/M/G suffix); small values force batch streaming")
    ap.add_argument("--max-batch-bytes", default="0", help="batch size of the streamed part of a shard (K/M/G suffix; default 128M)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: verification of every score, the CPU baseline, roofline / per-kernel "
                         "figures (HIP events, shader-clock sampling, device calibration), the Swiss-Prot-like secondary leg, the "
                         "peak sweep, the shard-proxy legs and the multi-rank weak-scaling run.  Without it a run sets up, warms "
                         "up, times --steps steps and prints the line; the --no-* switches below only matter with --full")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (per query: the merged top-K scores "
                         "and ids, the overflow / re-score counts) as DIR/<name>.npy in float64")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="peak workload: skip the Swiss-Prot-like secondary measurement")
    ap.add_argument("--no-sweep", action="store_true",
                    help="peak workload on one GPU: skip the peak-benchmark sweep (runpeakbenchmark.sh: 6 lengths x 4 kernel types)")
    ap.add_argument("--no-shard-proxy", action="store_true",
                    help="peak workload on one GPU: skip the shard-proxy legs (1/4 and 1/8 shards of both DBs, short-query streams)")
    ap.add_argument("--sweep-steps", type=int, default=2, help="timed passes per cell of the peak sweep (after one verified warm-up pass)")
    ap.add_argument("--no-families", action="store_true",
                    help="sprot-like workload: independent random residues only (the round-1..3 stand-in) instead of the DB with "
                         "seeded protein families of the queries")
    ap.add_argument("--cpu-sample-subjects", type=int, default=None)
    ap.add_argument("--db-prefix", default=os.environ.get("CUDASW4_SPROT_PREFIX"),
                    help="sprot-like workload (and the default run's secondary leg): a real DB made by `makedb` (e.g. "
                         "uniprot_sprot, runsprotbenchmark.sh:18-51) instead of the synthetic stand-in; default: "
                         "$CUDASW4_SPROT_PREFIX")
    ap.add_argument("--kernel-table", action="store_true",
                    help="with --full: add the per-kernel table of the timed region to the line (tools/collect_profiles.sh matches it with the PMC passes)")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if not args.full:
        args.no_cpu_baseline = args.no_verify = args.no_secondary = args.no_sweep = args.no_shard_proxy = True
    return args


def parse_size(s):
    s = str(s).strip()
    mult = {"K": 1 << 10, "M": 1 << 20, "G": 1 << 30}.get(s[-1:].upper(), 1)
    return int(float(s[:-1]) * mult) if mult > 1 else int(s)


def spawn_command(n, argv, port):
    """The command line that starts n ranks of this script (what the round driver runs itself for N > 1)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def spawn_ranks(n, argv):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.call(spawn_command(n, argv, port), env=env)


def kernel_source_sha():
    h = hashlib.sha256()
    for rel in KERNEL_SOURCES:
        with open(os.path.join(ROOT, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def load_counters():
    """PMC-derived constants (VALU instructions per cell pair, HBM traffic per launch) are only valid for the kernel
    sources they were measured on: profiles/kernel_counters.json records the sha of those sources; on a mismatch the
    fields are reported as null with a note instead of a stale number."""
    path = os.path.join(ROOT, "profiles", "kernel_counters.json")
    try:
        with open(path) as f:
            c = json.load(f)
    except (OSError, ValueError):
        return None, "profiles/kernel_counters.json missing"
    sha = kernel_source_sha()
    if c.get("kernel_src_sha16") != sha:
        return None, "profiles/kernel_counters.json was measured on kernel sources %s, these are %s: re-run tools/collect_profiles.sh" % (
            c.get("kernel_src_sha16"), sha)
    return c, None


def cpu_sample_of(num, ns, seed=1, longest=4):
    """Positions of the CPU leg's sample in a length-sorted DB of `num` subjects: `ns` uniformly drawn ones (ascending: a
    uniform draw of subjects is unbiased for residues per subject, so the leg measures the DB's rate) and, apart from them,
    the `longest` last ones (checked, not timed)."""
    rng = np.random.default_rng(seed)
    giants = np.arange(max(0, num - longest), num)
    pick = np.setdiff1d(rng.choice(num, min(ns, num), replace=False), giants)
    return pick, giants


def kinds_for(args):
    name = args.kernel or ("dpx" if args.workload == "sprot-like" else "half2")
    if name == "dpx":
        return name, (1, 1, 2, 2)
    k = KIND_BY_NAME[name]
    big = 3 if k in (0, 3) else 2
    small = k if k in (0, 1) else (0 if k == 3 else 1)
    return name, (k, small, big, big)


# ------------------------------------------------------------------------------------------------- CPU baseline
_CPU_THREADS = {}  # calibrated once per process: every CPU leg of a line uses the same team size


def pick_team(sweep):
    """{threads: rate} -> the team with the best SUSTAINED rate (ties within 2 %: the smaller team)"""
    top = max(sweep.values())
    return min(nt for nt, r in sweep.items() if r >= 0.98 * top)


def cpu_quota():
    """What the container may use: (cpus of the affinity mask, cgroup quota in cpus or None)."""
    try:
        ncpu = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        ncpu = os.cpu_count() or 1
    quota = None
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                parts = f.read().split()
            if path.endswith("cpu.max"):
                if parts and parts[0] != "max":
                    quota = float(parts[0]) / float(parts[1])
            else:
                q = float(parts[0])
                if q > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f2:
                        quota = q / float(f2.read().split()[0])
            break
        except (OSError, ValueError, IndexError):
            continue
    return ncpu, quota


def calibration_sample(chars, offsets, lengths, nt, blocks_per_thread=3, width=32):
    """The first subjects of a sample that give a team of nt threads `blocks_per_thread` blocks of `width` subjects each (the
    inter-sequence port scans 32 subjects in lock-step per block): work in proportion to the team, so that every team size
    of the sweep runs about equally long."""
    n = int(min(len(lengths), max(width, nt * blocks_per_thread * width)))
    return chars[:int(offsets[n] - offsets[0])], offsets[:n + 1], lengths[:n]


def calibrate_team(queries, chars, offsets, lengths, scan, max_threads, min_seconds=0.5):
    """Sustained rate of every team size max, max/2, ... 1 on the SAME work the leg is timed on — all queries of the set, in
    their own order, against a slice of the same sample sized in proportion to the team (calibration_sample) — repeated until
    at least `min_seconds` have gone by: several scheduler quota periods, not one burst.  Round 5 calibrated with ONE mid-length
    query on 6 000 subjects, a run of 7 ms at the larger team sizes: 611 GCUPS for 64 threads (830 for 128) in a container
    whose CPU quota then throttled the timed legs of the same team to 194 (100) — the sweep measured the burst, the legs the
    sustained rate, and short queries (whose blocks pay the per-column profile set-up over few rows) were not in it at all.
    -> {threads: GCUPS}"""
    sum_q = float(sum(len(q) for q in queries))
    sweep = {}
    nt = max_threads
    while nt >= 1:
        c, o, l = calibration_sample(chars, offsets, lengths, nt)
        res = float(l.astype(np.int64).sum())
        scan(queries[len(queries) // 2], c, o, l, nt)      # the team's threads exist and are warm
        cells, t0 = 0.0, time.perf_counter()
        while True:
            for q in queries:
                scan(q, c, o, l, nt)
            cells += sum_q * res
            dt = time.perf_counter() - t0
            if dt >= min_seconds:
                break
        sweep[nt] = cells / 1e9 / dt
        nt //= 2
    return sweep


def cpu_baseline(queries, chars, offsets, lengths, what, extra=None):
    """Oracle's SIMD scans (kind 'port') on the host cores over a bounded sample of the same workload: all 20 queries
    x the sample DB (pass it longest subjects first: the ports hand out blocks of consecutive subjects dynamically, and a
    block of 35 000-residue proteins taken last is a tail on one thread).  The team size comes from a sustained calibration on
    the same query mix (calibrate_team); `cores` reports the threads actually used, `cgroup_cpu_quota` what the container
    allows.  `extra`: further subjects (chars, offsets, lengths) that are scored for the checker but not timed (the longest
    proteins of a ragged DB).  Returns (json object, scores[query][subject] of the sample followed by the extra subjects) —
    the scores double as the checker of the GPU results."""
    import oracle_lib as O
    m = O.blosum21(62)
    qmid = queries[len(queries) // 2]

    def interseq(q, c, o, l, nt):
        return O.scan(q, c, o, l, m21=m, simd=True, nthreads=nt)
    if "n" not in _CPU_THREADS:
        sweep = calibrate_team(queries, chars, offsets, lengths, interseq, O.max_threads())
        _CPU_THREADS["n"] = pick_team(sweep)
        _CPU_THREADS["sweep"] = {str(k): round(v, 2) for k, v in sorted(sweep.items())}
    best_nt = _CPU_THREADS["n"]
    cells = float(sum(len(q) for q in queries)) * float(lengths.astype(np.int64).sum())
    rates, scores = {}, None
    for name, kw in (("striped", dict(striped=True)), ("interseq", dict(simd=True))):
        t0 = time.perf_counter()
        out = [O.scan(q, chars, offsets, lengths, m21=m, nthreads=best_nt, **kw) for q in queries]
        rates[name] = (cells / 1e9 / (time.perf_counter() - t0), time.perf_counter() - t0)
        if scores is not None and any((a != b).any() for a, b in zip(scores, out)):
            raise SystemExit("bench.py: the two CPU ports disagree")
        scores = out
    if extra is not None and len(extra[2]):
        more = [O.scan(q, *extra[:3], m21=m, nthreads=best_nt, simd=True) for q in queries]
        scores = [np.concatenate([a, b]) for a, b in zip(scores, more)]
    # the reference's own scalar int32 DP (cudasw4.cuh:2331-2392 restated), one core, a few hundred subjects
    ns = min(300, len(lengths))
    t0 = time.perf_counter()
    O.scan(qmid, chars[:int(offsets[ns] - offsets[0])], offsets[:ns + 1], lengths[:ns], m21=m, nthreads=1)
    scalar_rate = len(qmid) * float(lengths[:ns].astype(np.int64).sum()) / 1e9 / (time.perf_counter() - t0)
    model = ""
    try:
        with open("/proc/cpuinfo") as f:
            model = next((l.split(":", 1)[1].strip() for l in f if l.startswith("model name")), "")
    except OSError:
        pass
    best = max(rates, key=lambda k: rates[k][0])
    ncpu, quota = cpu_quota()
    obj = {"value": round(rates[best][0], 3), "unit": "GCUPS", "cores": best_nt, "kind": "port", "algorithm": best,
           "team_sweep_gcups": _CPU_THREADS.get("sweep"),
           "team_sweep_note": "sustained (>= 0.5 s per team size) inter-sequence rate on this query set against a slice of the "
                              "calibrating leg's sample in proportion to the team; the team with the best rate is used by every CPU leg of the process",
           "hardware_threads": O.max_threads(), "affinity_cpus": ncpu, "cgroup_cpu_quota": quota,
           "striped_gcups": round(rates["striped"][0], 3), "interseq_gcups": round(rates["interseq"][0], 3),
           "scalar_1core_gcups": round(scalar_rate, 4), "cpu_model": model,
           "sample": "%d queries x %s; oracle ports with int16 lanes (gcc, AVX-512 or AVX2 build picked by cpuid): Farrar "
                     "striped SW %.1f s, inter-sequence SIMD %.1f s; %d of %d hardware threads"
                     % (len(queries), what, rates["striped"][1], rates["interseq"][1], best_nt, O.max_threads())}
    return obj, scores


# ------------------------------------------------------------------------------------------------- device calibration
class SclkSampler:
    """Samples the shader clock the driver reports (sysfs pp_dpm_sclk: the level marked '*') every 50 ms while the timed
    region runs; None where the file cannot be read (no such node, no permission)."""

    def __init__(self, pci_bus_id=None):
        import glob
        self.path = None
        for cand in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
            if pci_bus_id:
                try:
                    slot = os.path.basename(os.path.realpath(os.path.dirname(cand)))
                except OSError:
                    slot = ""
                if pci_bus_id.lower() not in slot.lower():
                    continue
            self.path = cand
            break
        self.samples, self._stop, self._th = [], False, None

    def _read(self):
        try:
            with open(self.path) as f:
                for line in f:
                    if line.rstrip().endswith("*"):
                        return float(line.split(":")[1].lower().replace("mhz", "").replace("*", "").strip())
        except (OSError, ValueError, IndexError):
            return None
        return None

    def __enter__(self):
        if self.path and self._read() is not None:
            import threading

            def loop():
                while not self._stop:
                    v = self._read()
                    if v is not None:
                        self.samples.append(v)
                    time.sleep(0.05)
            self._th = threading.Thread(target=loop, daemon=True)
            self._th.start()
        return self

    def __exit__(self, *a):
        self._stop = True
        if self._th:
            self._th.join(timeout=1.0)

    def summary(self):
        if not self.samples:
            return None
        return {"source": self.path, "samples": len(self.samples), "min_mhz": min(self.samples),
                "avg_mhz": round(sum(self.samples) / len(self.samples), 1), "max_mhz": max(self.samples)}


MIX_BY_KIND = {0: (0, 3, 4), 1: (0, 3, 4), 2: (2,), 3: (1,)}   # sw_measure_valu_rate: packed kinds -> the best of the pure v_pk_maximum3_f16 stream and the kernels' own mix (two register placements); fp32 -> its co-issue mix; int32 -> its mix


def device_calibration(device):
    """What this very device issues and at which clock: CU count from the device, 50 ms in-process
    micro-runs of the three instruction mixes that bound the kinds' inner loops (capi.Context.measure_valu_rate =
    tools/ubench/valu_rate.hip / mix_rate.hip), the shader clock the waves of those runs saw.  Run right behind the timed
    region, on a warm chip."""
    import torch
    from cudasw4_amd import capi
    props = torch.cuda.get_device_properties(device)
    out = {"cus": int(props.multi_processor_count), "device": props.name, "mix": {}}
    try:
        ctx = capi.Context(device)
        for name, mix in (("vop3p_pk_maximum3_f16", 0), ("fp32_add_max3", 1), ("int32_add_max3", 2), ("packed_kernel_mix", 3), ("packed_kernel_mix_bank_free", 4)):
            rate, hz = ctx.measure_valu_rate(mix, 50)
            out["mix"][str(mix)] = {"name": name, "lane_instr_per_s": rate,
                                    "lanes_per_clk_per_cu_at_2.4GHz": round(rate / (out["cus"] * 2.4e9), 2),
                                    "shader_clock_hz": hz if 0.5e9 < hz < 4e9 else None}
        ctx.close()
    except Exception as e:  # the figures below then stay nominal, and say so
        out["error"] = str(e)[:200]
    return out


def valu_peaks(kind, cal, sclk):
    """-> (nominal peak, measured peak or None, peak at the observed clock or None) in lane-instructions per second.
    nominal: CUs of THIS device x the kind's issue ceiling in lanes/clk/CU (profiles/r01_valu_rate.txt, r01_mix_rate.txt) x
    2.4 GHz; measured: the micro-run's own rate; observed clock: the nominal ceiling at the average shader clock sampled
    during the timed region."""
    lanes_per_clk = {0: 64.0, 1: 64.0, 2: 5.75 / (2.25 / 98.0 + 3.5 / 64.0), 3: 99.5}[kind]
    cus = (cal or {}).get("cus") or 256
    nominal = cus * lanes_per_clk * 2.4e9
    rates = [(((cal or {}).get("mix") or {}).get(str(m)) or {}).get("lane_instr_per_s") for m in MIX_BY_KIND[kind]]
    measured = max([r for r in rates if r], default=None)
    at_clock = cus * lanes_per_clk * sclk["avg_mhz"] * 1e6 if sclk and sclk.get("avg_mhz") else None
    return nominal, measured, at_clock, lanes_per_clk, cus


# ------------------------------------------------------------------------------------------------- roofline
def union_ms(intervals):
    """Measure of the union of (begin, end) intervals: the time at least one of them was running."""
    total, cur_b, cur_e = 0.0, None, None
    for b, e in sorted(intervals):
        if cur_e is None or b > cur_e:
            if cur_e is not None:
                total += cur_e - cur_b
            cur_b, cur_e = b, e
        else:
            cur_e = max(cur_e, e)
    if cur_e is not None:
        total += cur_e - cur_b
    return total


def kernel_name_of(e):
    """swk::sw_scan_kernel's template arguments as rocprofv3 prints them (the last one, the form of the recurrence, is
    left open: it follows from the gap scores, not from the launch)."""
    return "sw_scan_kernel<%d, %d, %d, %s," % (e["eff_kind"], e["rows"], e["lanes"], "true" if e["nstripes"] > 1 else "false")


def residency_of(info):
    if info["resident"]:
        return "resident"
    return "hybrid" if info.get("cached_chars", 0) > 0 else "streamed"


def counters_key(workload, kernel_name, residency):
    return "%s:%s:%s%s" % (workload, kernel_name, residency, ":i32native" if os.environ.get("CUDASW4_AMD_I32_NATIVE") == "1" else "")


def roofline_objects(args, workload, kernel_name, events, info, cal=None, sclk=None):
    """`roofline` (the HBM view the contract asks for), `valu_roofline` (the binding bound) and the per-kernel table of
    the timed region, from the HIP events the driver recorded around every DP launch on the stream it ran on.

    * the dominant kernel is the instantiation that computed the most cells; `achieved` = its algorithmic bytes
      per launch / its average launch duration;
    * `traffic` = the PMC-measured HBM-side bytes PER SUBJECT BYTE of that instantiation (profiles/kernel_counters.json)
      x the subject bytes of an average launch here — a launch of a 128 MB batch is not charged with the traffic of a
      532 MB one;
    * the DP kernels' own rate (`kernel_gcups`) = cells / the measure of the UNION of all launch intervals: launches
      overlap (long subjects on the auxiliary streams, consecutive batches on two work streams), a sequence of batches
      does not — neither the sum nor the longest launch of a scan is the time the kernels took."""
    all_events = events
    events = [e for e in all_events if not e.get("rescore")]  # the re-score launches count as busy time, not as cells
    if not events:
        return None, None, []
    groups = {}
    for e in events:
        groups.setdefault(kernel_name_of(e), []).append(e)
    ktable = [{"kernel": k + " *>", "launches": len(v), "total_ms": round(sum(e["ms"] for e in v), 3),
               "chars": int(sum(e["chars"] for e in v)), "cells": float(sum(e["cells"] for e in v)),
               "nstripes": sorted(set(e["nstripes"] for e in v))} for k, v in sorted(groups.items())]
    # (by cells, not by summed launch time: the side launch of a real DB's few giants runs for as long as the bulk launch it
    # hides behind and does a thousandth of the work — round 6: it was picked for the Swiss-Prot-like leg and priced the packed
    # kernels' instructions per cell PAIR as per cell)
    key = max(groups, key=lambda k: sum(e["cells"] for e in groups[k]))
    ev = groups[key]
    kind = ev[0]["eff_kind"]
    avg_ms = sum(e["ms"] for e in ev) / len(ev)
    avg_chars = sum(e["chars"] for e in ev) / len(ev)
    # algorithmic HBM bytes of one launch: chars + lengths + offsets + scores/ids + query
    bytes_per_launch = sum(e["chars"] + 4 * e["subjects"] + 8 * (e["subjects"] + 1) + 8 * e["subjects"] + (e["qlen"] + 3) // 4 * 4 + 128
                           for e in ev) / len(ev)
    hbm_gbs = bytes_per_launch / 1e9 / (avg_ms * 1e-3)
    counters, cnote = load_counters()
    lanes = ev[0]["lanes"]
    kname = "sw_scan_kernel<%s, R=%d, %d lanes, %s>" % (DTYPE_BY_KIND[kind], ev[0]["rows"], lanes,
                                                        "multi-stripe" if ev[0]["nstripes"] > 1 else "single stripe")
    traffic, tnote = None, cnote
    if counters:
        t = (counters.get("traffic_bytes_per_char") or {}).get("%s|%s" % (workload, key))
        if t and sorted(set(e["nstripes"] for e in ev)) == t.get("nstripes"):
            traffic = int(t["value"] * avg_chars)
            tnote = "%.2f HBM-side bytes per subject byte of this instantiation (%s) x %d subject bytes per launch here" % (
                t["value"], t["source"], int(avg_chars))
        else:
            tnote = "no PMC traffic figure for %s *> with these stripes" % key
    busy_ms = union_ms([(e["t0_ms"], e["t1_ms"]) for e in all_events])
    roof = {"bound": "hbm", "achieved": round(hbm_gbs, 3), "peak": 8000.0, "unit": "GB/s",
            "peak_note": "MI355X HBM3E, /opt/skills/guides/MI355X_MICROARCH.md; this path moves 0.0005 bytes per cell (SURVEY.md 8d)",
            "frac": round(hbm_gbs / 8000.0, 6), "traffic": traffic, "kernel": kname,
            "avg_launch_ms": round(avg_ms, 4), "launches": len(ev), "algorithmic_bytes_per_launch": int(bytes_per_launch),
            "share_of_kernel_time": round(sum(e["ms"] for e in ev) / sum(e["ms"] for e in events), 3)}
    if tnote:
        roof["traffic_note"] = tnote
    # the binding bound: VALU issue.  Peak: one wave64 instruction per 4 cycles per SIMD =
    # 64 lanes/clk/CU, 256 CUs at 2.4 GHz; fp32 kind: v_add_f32 co-issues with v_max3_f32 (99.5 lanes/clk/CU)
    packed = kind in (0, 1)
    kern_gcups = sum(e["cells"] for e in events) / 1e9 / (busy_ms * 1e-3)
    # lanes/clk/CU the kind's instruction mix can issue at best (tools/ubench/valu_rate.hip, mix_rate.hip):
    # packed 16-bit ops are VOP3P, one wave64 instruction per 4 cycles per SIMD = 64; the fp32 kind's v_add_f32 co-issues
    # with v_max3_f32: 99.5 for its 8:7 mix; the int32 kind cannot co-issue, but its v_add_u32 (VOP2) issue at 98 when alone
    # and its v_max3_i32 at 64: 2.25 adds + 3.5 max3 per cell -> 5.75 / (2.25 / 98 + 3.5 / 64) = 74
    valu_peak, peak_measured, peak_at_clock, lanes_per_clk, cus = valu_peaks(kind, cal, sclk)
    residency = residency_of(info)
    ipu, ipu_key = None, None
    if counters:
        table = counters.get("valu_instr_per_unit") or {}
        for r in (residency, "resident"):
            ipu_key = counters_key(workload, kernel_name, r)
            if ipu_key in table:
                ipu = table[ipu_key]
                break
    valu = {"bound": "valu-issue", "peak": round(valu_peak / 1e12, 3), "unit": "T lane-instr/s",
            "kernel_gcups": round(kern_gcups, 1), "kernel_busy_ms_per_step": round(busy_ms / max(args.steps, 1), 3),
            "note": "the binding bound of this path (DESIGN.md §3): the DP recurrence is VALU-issue bound, not HBM "
                    "bound; roofline.frac above is the HBM view the contract asks for.  kernel_gcups = cells / union of "
                    "the launches' HIP-event intervals"}
    valu.update({"cus": cus, "lanes_per_clk_per_cu": round(lanes_per_clk, 2), "nominal_clock_ghz": 2.4,
                 "peak_measured": round(peak_measured / 1e12, 3) if peak_measured else None,
                 "peak_at_observed_clock": round(peak_at_clock / 1e12, 3) if peak_at_clock else None,
                 "observed_sclk": sclk, "calibration": cal,
                 "peak_measured_note": "lane-instructions per second of the best of the 50 ms in-process micro-runs of the kind's bounding mix on THIS "
                                       "device (packed kinds: a pure v_pk_maximum3_f16 stream, and the instruction histogram of the dominant loop "
                                       "body — 55 % v_pk_maximum3_f16, 16 % v_pk_fma_f16, 20 % v_pk_add_f16, 9 % DPP / v_add_u32 — with operands "
                                       "where the allocator puts them and with every instruction's sources in three register banks: "
                                       "sw_measure_valu_rate mixes 0, 3, 4).  A FLOOR of what the chip can issue, not a ceiling: the scan kernels — "
                                       "three waves per SIMD from different workgroups, their 9 % of VOP1/VOP2 instructions issued at the faster "
                                       "rate — sustain 2-3 % more than any micro-run (frac_of_measured_peak > 1).  The bound they cannot beat is "
                                       "peak_at_observed_clock = 64 lanes/clk/CU x CUs x the sampled shader clock (frac_at_observed_clock)",
                 "lanes_per_clk_note": "`frac` prices the achieved rate against 64 lanes/clk/CU (one VOP3/VOP3P wave64 instruction per 4 "
                                       "cycles per SIMD, the measured issue rate of every packed, 3-input and DPP op: profiles/r01_valu_rate.txt) "
                                       "x CUs x the nominal 2.4 GHz; `frac_of_128` against the guide's SIMD-32 rate (128 lanes/clk/CU = the 157 TF "
                                       "fp32 vector peak, MI355X_MICROARCH.md:52-54), which only plain VOP2 fp32/int32 ops approach (98 "
                                       "measured) and no packed 16-bit, 3-input or DPP op does: two packed cells per instruction at 62 lanes/clk "
                                       "beat one 16-bit cell per VOP2 instruction at 100"})
    if ipu:
        ach = kern_gcups * 1e9 / (2 if packed else 1) * ipu["value"]
        valu.update({"frac_of_measured_peak": round(ach / peak_measured, 4) if peak_measured else None,
                     "frac_at_observed_clock": round(ach / peak_at_clock, 4) if peak_at_clock else None})
        valu.update({"achieved": round(ach / 1e12, 3), "frac": round(ach / valu_peak, 4),
                     "frac_of_128": round(ach / (cus * 128.0 * 2.4e9), 4),
                     "instr_per_cell_pair" if packed else "instr_per_cell": ipu["value"],
                     "counters": ipu["source"], "counters_key": ipu_key})
    else:
        valu.update({"achieved": None, "frac": None,
                     "counters_note": cnote or "no PMC figure for %s" % counters_key(workload, kernel_name, residency)})
    return roof, valu, ktable


# ------------------------------------------------------------------------------------------------- one rank
def run_rank(args):
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # BENCH_FORCE_DIST=1 (test hook): go through the process-group code path (RCCL init, gather, reductions, barrier) even
    # with a single rank, which is all a 1-GPU box can run with the real backend
    distributed = world > 1 or os.environ.get("BENCH_FORCE_DIST") == "1"
    if os.environ.get("BENCH_FAIL_RANK") == str(rank):
        # test hook: a rank that dies (before it touches the GPU) must take the whole job down with a non-zero exit code
        sys.stderr.write("bench.py: rank %d fails on request (BENCH_FAIL_RANK)\n" % rank)
        sys.exit(3)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product has no CPU path")
    # test hooks (1-GPU boxes): BENCH_FORCE_DEVICE maps every rank onto one device, BENCH_DIST_BACKEND=gloo
    # replaces RCCL (which refuses two ranks on one GPU).  The driver's multi-GPU runs use neither.
    if "BENCH_FORCE_DEVICE" in os.environ:
        local_rank = int(os.environ["BENCH_FORCE_DEVICE"])
    backend = os.environ.get("BENCH_DIST_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    comm_dev = torch.device("cuda", local_rank) if backend == "nccl" else torch.device("cpu")
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)

    # one process per GPU: this rank's threads (the driver's launches, its staging copies of streamed shards) run on the
    # NUMA node the GPU hangs off — on a two-socket box half of the GPUs sit behind the other socket
    from cudasw4_amd import driver as _driver
    numa_node = _driver.device_numa_node(local_rank)
    numa_bound = os.environ.get("BENCH_NO_NUMA_BIND") != "1" and _driver.bind_to_numa_node(numa_node)
    sys.stderr.write("bench.py: rank %d of %d on GPU %d, NUMA node %d%s\n" % (rank, world, local_rank, numa_node, " (threads bound to it)" if numa_bound else ""))

    class Env:
        pass
    env = Env()
    env.numa_node, env.numa_bound = numa_node, bool(numa_bound)
    env.torch, env.dist, env.world, env.rank, env.local_rank = torch, dist, world, rank, local_rank
    env.distributed, env.backend, env.comm_dev = distributed, backend, comm_dev
    out = measure(env, args, args.workload, want_cpu=not args.no_cpu_baseline and world == 1, dump_dir=args.dump_outputs)
    if args.workload == "peak" and not args.no_secondary:
        # BASELINE config 3 under the same clock: the Swiss-Prot-like DB with the packed-int16 configuration, reported
        # next to the headline (its own timed region, verification and roofline; the CPU leg doubles as its checker)
        import copy
        a2 = copy.copy(args)
        a2.workload, a2.kernel, a2.db_size, a2.cpu_sample_subjects = "sprot-like", None, None, None
        sec = measure(env, a2, "sprot-like", want_cpu=not args.no_cpu_baseline and world == 1)
        if rank == 0:
            out["sprot_like"] = {k: sec[k] for k in ("value", "unit", "ms_per_step", "scaling", "dtype", "data", "verified", "verified_how",
                                                      "config", "roofline", "valu_roofline", "overflow_load", "cpu_baseline") if k in sec}
    if args.workload == "peak" and world == 1 and not args.no_sweep and not args.no_secondary:
        sweep = peak_sweep(env, args)
        if rank == 0:
            out["peak_sweep"] = sweep
    if args.workload == "peak" and world == 1 and not args.no_shard_proxy and not args.no_secondary and args.db_length == 512 and not args.db_size:
        proxy, short = shard_proxy(env, args, out["value"])
        if rank == 0:
            out["shard_proxy"] = proxy
            out["short_queries"] = short
    if distributed and world > 1 and args.scaling == "strong" and args.workload == "peak" and not args.no_secondary:
        # next to the strong-scaling headline (ONE DB sharded over the ranks): the same benchmark with one full DB per
        # rank, so that a multi-GPU run shows both what sharding a 532 MB DB eight ways costs and what the GPUs do when
        # each keeps a full-size shard
        import copy
        a3 = copy.copy(args)
        a3.scaling = "weak"
        wk = measure(env, a3, "peak", want_cpu=False)
        if rank == 0:
            out["weak_scaling"] = {k: wk[k] for k in ("value", "unit", "ms_per_step", "scaling", "verified", "config") if k in wk}
    if rank == 0:
        print(json.dumps(out))
        sys.stdout.flush()
    if distributed:
        dist.destroy_process_group()


_DB_CACHE = {}


def sprot_db(n, families=True):
    """The Swiss-Prot-like DB of n sequences (seeded: the same arrays for every leg of a line)."""
    from cudasw4_amd import synthdb
    key = (int(n), bool(families))
    if key not in _DB_CACHE:
        _DB_CACHE[key] = synthdb.sprot_like(int(n), families=bool(families))
    return _DB_CACHE[key]


def shard_proxy(env, args, full_peak_gcups):
    """What ONE rank of an N-GPU run gets from the two benchmark DBs, measured on one GPU (SCALE stays a
    skipped record while no multi-GPU node is available): the Swiss-Prot-like DB at 1/1, 1/4 and 1/8 of the subjects — same
    length distribution, EVERY one holding the 35 213-residue giant, i.e. the rank that gets titin — and the peak DB at 1/8
    (125 000 x 512); all 20 queries, walked the way `align` walks a query file (Driver.scan_stream: the driver's own
    in-flight rule — two queries in flight on a small resident shard, one on a large one), top-K inside the timed region.
    Per leg: one warm-up pass in which EVERY score is checked (peak: the reference's golden score; Swiss-Prot-like: the CPU
    oracle on a seeded sample plus the four longest subjects) and the top-K lists against the top of all scores, then
    `passes` timed passes.  Reported as GCUPS and as fraction of the full-DB rate (the 1/1 leg here; the headline for the
    peak DB).  Plus `short_queries`: streams of 16 random 48- / 96-residue queries on the full Swiss-Prot-like DB, one at a
    time and by the driver's rule, every top-10 list equal between the two modes."""
    torch = env.torch
    from cudasw4_amd import driver, search, synthdb
    import oracle_lib as O   # the checker of the warm-up passes, nothing of it is timed
    _, query_letters = driver.read_sequences(os.path.join(ROOT, "tests", "golden", "allqueries.fasta"))
    queries = [driver.encode(q) for q in query_letters]
    sum_q = float(sum(len(q) for q in queries))
    K = max(args.top, 0)
    passes = 3
    m62 = O.blosum21(62)
    nt = _CPU_THREADS.get("n", 0)
    t_begin = time.perf_counter()

    def top_of_all(sc, ids, k):
        kk = min(k, len(sc))
        thr = np.partition(sc, len(sc) - kk)[len(sc) - kk]
        cand = np.nonzero(sc >= thr)[0]
        return search.merge_topk([(sc[cand], ids[cand])], kk)

    def timed(drv, qs, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn(qs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    legs, ok_all = [], True
    full_rate = {}
    short = None
    for workload, denom in (("sprot-like", 1), ("sprot-like", 4), ("sprot-like", 8), ("peak", 8)):
        if workload == "peak":
            num, kinds = 1_000_000 // denom, (0, 0, 3, 3)
            drv = driver.Driver(devices=[env.local_rank], num_top=K, matrix=62, kinds=kinds)
            drv.pseudo_db(num, 512)
            residues = float(num) * 512
            golden = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_scores.json")))["pseudo"]["512"]
        else:
            num, kinds = synthdb.SPROT_SEQUENCES // denom, (1, 1, 2, 2)
            chars, offsets, lengths = sprot_db(num)
            drv = driver.Driver(devices=[env.local_rank], num_top=K, matrix=62, kinds=kinds)
            drv.db_from_arrays(chars, offsets, lengths)
            residues = float(lengths.astype(np.int64).sum())
            pick, giants = cpu_sample_of(num, 1500, seed=3)
            pick = np.concatenate([pick, giants])
            sub = search.build_shard(chars, offsets, lengths, [(int(i), int(i) + 1) for i in pick[::-1]])
        drv.upload()
        ok = True
        tops = []
        for qi, q in enumerate(query_letters):   # warm-up pass == verification pass
            r = drv.scan(q)
            ids, sc = drv.all_scores()
            if workload == "peak":
                ok = ok and len(sc) == num and int(sc.min()) == int(sc.max()) == int(golden[qi])
            else:
                want = O.scan(queries[qi], *sub[:3], m21=m62, simd=True, nthreads=nt)
                by_id = np.empty(num, dtype=np.int32)
                by_id[ids] = sc
                ok = ok and len(sc) == num and (by_id[pick[::-1]] == want).all()
            if K > 0:
                top = top_of_all(sc, ids, K)
                ok = ok and r["scores"].tolist() == top[0].tolist() and r["ids"].tolist() == top[1].tolist()
                tops.append((r["scores"].tolist(), r["ids"].tolist()))
        drv.scan_stream(query_letters)   # the lanes of two queries in flight are warm as well
        before = drv.tail_overlaps()
        best = 1e30
        for _ in range(passes):
            dt, res = timed(drv, query_letters, drv.scan_stream)
            best = min(best, dt)
            if K > 0:
                ok = ok and [(r["scores"].tolist(), r["ids"].tolist()) for r in res] == tops
        rate = sum_q * residues / 1e9 / best
        if denom == 1:
            full_rate[workload] = rate
        base = full_rate.get(workload) or (full_peak_gcups if workload == "peak" else None)
        legs.append({"db": workload, "shard": "1/%d" % denom, "subjects": num, "residues": int(residues), "gcups": round(rate, 1),
                     "frac_of_full_db_rate": round(rate / base, 4) if base else None, "ms_per_pass": round(best * 1e3, 2),
                     "two_in_flight": bool(drv.prefers_two_in_flight()),
                     "gated_queries_per_pass": (drv.tail_overlaps() - before) // passes, "verified": bool(ok)})
        ok_all = ok_all and bool(ok)
        if workload == "sprot-like" and denom == 1:
            # streams of short queries on the same driver / DB
            rng = np.random.default_rng(1)
            alphabet = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)
            short = {"unit": "GCUPS", "db": "Swiss-Prot-like, %d subjects, dpx kernels" % num, "queries_per_stream": 16, "lengths": {}}
            for n in (48, 96):
                qs = [alphabet[rng.integers(0, 20, n)].tobytes() for _ in range(16)]
                enc0 = driver.encode(qs[0])
                drv.scan(qs[0])
                ids, sc = drv.all_scores()
                by_id = np.empty(num, dtype=np.int32)
                by_id[ids] = sc
                sok = bool((by_id[pick[::-1]] == O.scan(enc0, *sub[:3], m21=m62, simd=True, nthreads=nt)).all())
                one_at_a_time = lambda L: [drv.scan(q) for q in L]
                drv.scan_stream(qs)
                t_alone, t_stream, lists = 1e30, 1e30, []
                for _ in range(3):
                    dt, res = timed(drv, qs, one_at_a_time)
                    t_alone = min(t_alone, dt)
                    lists.append([(r["scores"].tolist(), r["ids"].tolist()) for r in res])
                    dt, res = timed(drv, qs, drv.scan_stream)
                    t_stream = min(t_stream, dt)
                    lists.append([(r["scores"].tolist(), r["ids"].tolist()) for r in res])
                sok = sok and all(l == lists[0] for l in lists)
                short["lengths"][str(n)] = {"one_at_a_time": round(n * 16 * residues / 1e9 / t_alone, 1),
                                            "drivers_rule": round(n * 16 * residues / 1e9 / t_stream, 1),
                                            "two_in_flight_by_rule": bool(drv.prefers_two_in_flight(n)), "verified": sok}
                ok_all = ok_all and sok
        drv.close()
    return {"unit": "GCUPS", "legs": legs, "verified": bool(ok_all), "passes": passes,
            "protocol": "one GPU; per leg a driver of its own, DB resident, 1 verified warm-up pass (every score of every query: peak = "
                        "golden score, Swiss-Prot-like = CPU oracle on 1 500 sampled subjects + the 4 longest; top-%d == top of all scores), "
                        "then the best of %d timed passes of the 20 queries through Driver.scan_stream (what `align` does: two queries in "
                        "flight where the driver's rule says so); every Swiss-Prot-like shard holds the 35 213-residue giant" % (K, passes),
            "seconds": round(time.perf_counter() - t_begin, 1)}, short


def peak_sweep(env, args):
    """The reference's peak protocol (runpeakbenchmark.sh:26-83) under the same clock as the headline: allqueries.fasta
    against `--pseudodb 1000000 L` for L in {128, 256, 512, 768, 1024, 2048} x {half2, dpxs16} and L <= 1024 x {dpxs32,
    float}, resident, through the C++ driver.  Per cell: ONE warm-up pass in which every score of every query is checked
    against the reference's golden score (tests/golden/ref_scores.json), then --sweep-steps timed passes bracketed by
    device synchronisation (top-K inside, like the headline).  The headline's own cell (half2, 512) is measured again
    here with the sweep's few steps."""
    torch = env.torch
    from cudasw4_amd import driver
    _, query_letters = driver.read_sequences(os.path.join(ROOT, "tests", "golden", "allqueries.fasta"))
    sum_q = sum(len(q) for q in query_letters)
    golden_all = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_scores.json")))["pseudo"]
    num = args.db_size or 1_000_000
    K = max(args.top, 0)
    table, ok_all, t_begin = {}, True, time.perf_counter()
    import copy
    for kname, lengths in (("half2", (128, 256, 512, 768, 1024, 2048)), ("dpxs16", (128, 256, 512, 768, 1024, 2048)),
                           ("dpxs32", (128, 256, 512, 768, 1024)), ("float", (128, 256, 512, 768, 1024))):
        a = copy.copy(args)
        a.kernel, a.workload = kname, "peak"
        _, kinds = kinds_for(a)
        row = {}
        for L in lengths:
            golden = golden_all.get(str(L))
            drv = driver.Driver(devices=[env.local_rank], num_top=K, matrix=62, kinds=kinds)
            drv.pseudo_db(num, L)
            drv.upload()
            ok = golden is not None
            for qi, q in enumerate(query_letters):  # warm-up pass == verification pass
                drv.scan(q)
                sc, _ids = drv.last_scores(0)
                ok = ok and len(sc) == num and int(sc.min()) == int(sc.max()) == int(golden[qi])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(max(args.sweep_steps, 1)):
                drv.scan_stream(query_letters)   # the way `align` walks a query file (one at a time, two where the driver's rule says so)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            drv.close()
            row[str(L)] = round(float(sum_q) * num * L * max(args.sweep_steps, 1) / 1e9 / dt, 1)
            ok_all = ok_all and bool(ok)
        table[kname] = row
    return {"unit": "GCUPS", "protocol": "runpeakbenchmark.sh:26-83: allqueries.fasta x pseudo DB %d x L, resident, blosum62, gop -11 gex -1, "
                                        "top %d, C++ host driver, queries walked like `align` does (Driver.scan_stream); per cell 1 verified warm-up pass + %d timed passes" % (num, K, max(args.sweep_steps, 1)),
            "gcups": table, "verified": ok_all,
            "verified_how": "in every cell all %d scores of each of the 20 queries equal the reference's golden score" % num,
            "dpxs32_note": "int32 results computed in fp32 lanes (exact below 2^24, bound checked per launch)"
                           if os.environ.get("CUDASW4_AMD_I32_NATIVE") != "1" else "native int32 kernels",
            "seconds": round(time.perf_counter() - t_begin, 1)}


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(dump_dir, results, merged, K):
    """--dump-outputs: what the last timed step handed its caller, per query — the merged top-K scores and ids (-1 where a
    list is shorter than K) and this rank's overflow / re-score counts — as float64 DIR/<name>.npy.  Were the top-K lists
    above 64 MB in all, a fixed, seeded sample of their columns is written instead."""
    nq = len(results)
    scores, ids = np.full((nq, K), -1.0), np.full((nq, K), -1.0)
    for qi in range(nq if K > 0 else 0):
        s, i = merged[qi]
        scores[qi, :len(s)] = s
        ids[qi, :len(i)] = i
    cols = max(1, (DUMP_BUDGET_BYTES - (1 << 20)) // (16 * max(nq, 1)))   # (1 MB for the counts and the .npy headers)
    if K > cols:
        keep = np.sort(np.random.default_rng(0).choice(K, cols, replace=False))
        scores, ids = scores[:, keep], ids[:, keep]
    os.makedirs(dump_dir, exist_ok=True)
    arrays = {"top_scores": scores, "top_ids": ids,
              "num_overflows": np.array([r["num_overflows"] for r in results], dtype=np.float64),
              "num_rescored": np.array([r["num_rescored"] for r in results], dtype=np.float64)}
    for name, a in arrays.items():
        np.save(os.path.join(dump_dir, name + ".npy"), a)


def measure(env, args, workload, want_cpu, dump_dir=None):
    """One workload on this rank: load the DB shard, warm up, time `steps` steps, write the last step's results to
    `dump_dir` (rank 0), verify every score (--full), build the JSON object (returned on rank 0, None elsewhere)."""
    torch, dist, world, rank, local_rank = env.torch, env.dist, env.world, env.rank, env.local_rank
    distributed, comm_dev = env.distributed, env.comm_dev
    # inputs come from the product's own host library (FASTA reader, encoder, pseudo-DB generator);
    # oracle/ is touched only inside cpu_baseline()
    from cudasw4_amd import capi, driver, search, synthdb

    _, query_letters = driver.read_sequences(os.path.join(ROOT, "tests", "golden", "allqueries.fasta"))
    query_index = list(range(len(query_letters)))   # positions in allqueries.fasta (the golden scores are per file position)
    if args.queries:
        query_index = [int(i) for i in args.queries.split(",")]
        query_letters = [query_letters[i] for i in query_index]
    queries = [driver.encode(q) for q in query_letters]
    sum_q = sum(len(q) for q in queries)
    kernel_name, kinds = kinds_for(args)
    strong = args.scaling == "strong" or not distributed
    K = max(args.top, 0)

    nshards = max(1, args.shards_per_gpu)
    drv = driver.Driver(devices=[local_rank] * nshards, num_top=K, matrix=62, kinds=kinds, max_gpu_mem=parse_size(args.max_gpu_mem),
                        max_batch_bytes=parse_size(args.max_batch_bytes))
    host_db = None
    data = "synthetic"
    if args.workload == "peak":
        num = args.db_size or 1_000_000
        L = args.db_length
        drv.set_shard(rank, world, 0) if strong else drv.set_shard(0, 1, rank * num)
        drv.pseudo_db(num, L)
        total_residues = float(num) * L * (1 if strong else world)
        total_subjects = num * (1 if strong else world)
        what = "pseudo DB %d x %d%s" % (num, L, "" if strong else " per GPU")
    else:
        if args.db_prefix:
            # a real DB in dbdata layout (makedb's output): the driver memory-maps it like `align`; the CPU leg and the
            # verification read the same files
            chunk = args.db_prefix + "0"
            host_db = (np.memmap(chunk + "chars", dtype=np.int8, mode="r"), np.fromfile(chunk + "offsets", dtype=np.uint64),
                       np.fromfile(chunk + "lengths", dtype=np.int32))
            num = len(host_db[2])
            drv.set_shard(rank, world, 0) if strong else drv.set_shard(0, 1, rank * num)
            drv.open_db(args.db_prefix, prefetch=True)
            data = "real"
            label = "DB %s" % args.db_prefix
        elif args.workload in ("uniref50-like", "trembl-like"):
            # trembl-like: BASELINE config 5 at its own size (runtremblbenchmark.sh:21: ~2.5e8 sequences, 9e10 residues) —
            # the same generator, 2.5e8 sequences: 96 GB of chars, ids within 12 % of INT32_MAX
            num = args.db_size or (synthdb.TREMBL_SEQUENCES if args.workload == "trembl-like" else synthdb.UNIREF50_SEQUENCES)
            t_gen = time.perf_counter()
            host_db = synthdb.uniref50_like(num, torch_device=torch.device("cuda", local_rank))
            drv.set_shard(rank, world, 0) if strong else drv.set_shard(0, 1, rank * num)
            drv.db_from_arrays(*host_db)
            label = ("TrEMBL-sized" if args.workload == "trembl-like" else "UniRef50-sized") + " synthetic DB (Swiss-Prot length histogram and composition, independent residues; generated and loaded in %.0f s)" % (
                time.perf_counter() - t_gen)
        else:
            num = args.db_size or synthdb.SPROT_SEQUENCES
            host_db = sprot_db(num, families=not args.no_families)
            drv.set_shard(rank, world, 0) if strong else drv.set_shard(0, 1, rank * num)
            drv.db_from_arrays(*host_db)
            label = "Swiss-Prot-like synthetic DB (Swiss-Prot composition%s)" % (
                "" if args.no_families else ", seeded families of the 20 queries: mutated copies, fragments, domains in foreign flanks")
        total_residues = float(host_db[2].astype(np.int64).sum()) * (1 if strong else world)
        total_subjects = num * (1 if strong else world)
        what = "%s (%d sequences, %d residues, %s, max %d)%s" % (
            label, num, int(host_db[2].astype(np.int64).sum()), "lengths as in the file" if args.db_prefix else "log-normal lengths",
            int(host_db[2].max()), "" if strong else " per GPU")
    drv.upload()
    info = drv.shard_info(0)

    merged = [None] * len(queries)
    load = {"num_overflows": 0, "num_rescored": 0}  # of the last step: summed over its 20 queries (this rank's shard)
    last = {}  # the last step's per-query results on this rank (--dump-outputs)
    # "always": every query submitted before the one before it is collected (multi-rank runs: small shards); "never": one
    # at a time; "rule": like `align` — two in flight exactly where the driver says the tail hand-over applies
    # (Driver.scan_stream: small resident shards, queries that are scanned in a few milliseconds)
    pipelined = os.environ["BENCH_PIPELINE"] == "1" if "BENCH_PIPELINE" in os.environ else (world > 1 or drv.prefers_two_in_flight())
    by_rule = "BENCH_PIPELINE" not in os.environ and not pipelined

    def one_step():
        """20 scans through the C++ driver (each returns this rank's top-K on the host), then ONE exchange of the
        per-rank lists — K (score, id) pairs per query and rank — and the host-side merge on rank 0."""
        mine = np.full((len(queries), max(K, 1), 2), -1, dtype=np.int64)
        # One query at a time, like the reference (main.cu:217-260), on one GPU; with several ranks — small shards, where
        # the fixed work per query weighs more — the driver takes the next query while the current one's top-K is still
        # on its way back (Driver.scan_many, SearchDriver::submit / collect), and on a small resident shard the next
        # query's launch fills the slots the current one's last round leaves idle (tail hand-over: swdrv_tail_overlaps).
        # Measured on one GPU: 125 000-subject shard 10.83 -> 11.28 TCUPS, +-0.1 % on the 10^6 x 512 DB (no hand-over
        # there), -0.1 ... -0.6 % on the Swiss-Prot-like DB.  BENCH_PIPELINE=0|1 forces it.
        results = drv.scan_many(query_letters) if pipelined else drv.scan_stream(query_letters) if by_rule else [drv.scan(q) for q in query_letters]
        load["num_overflows"] = sum(r["num_overflows"] for r in results)
        load["num_rescored"] = sum(r["num_rescored"] for r in results)
        last["results"] = results
        for qi, r in enumerate(results):
            n = len(r["scores"])
            mine[qi, :n, 0] = r["scores"]
            mine[qi, :n, 1] = r["ids"]
        if K == 0:
            return
        if distributed:
            t = torch.from_numpy(mine).to(comm_dev)
            parts = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(parts, t)
            if rank == 0:
                allp = [p.cpu().numpy() for p in parts]
                for qi in range(len(queries)):
                    lists = [(p[qi, :, 0][p[qi, :, 1] >= 0], p[qi, :, 1][p[qi, :, 1] >= 0]) for p in allp]
                    merged[qi] = search.merge_topk(lists, K)
        else:
            for qi in range(len(queries)):
                keep = mine[qi, :, 1] >= 0
                merged[qi] = search.merge_topk([(mine[qi, keep, 0], mine[qi, keep, 1])], K)

    def barrier():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        one_step()
    barrier()
    h2d_before = drv.streamed_bytes()
    # --full: HIP events around every DP launch and the shader clock sampled during the timed region (roofline figures)
    sclk_sampler = contextlib.nullcontext()
    if args.full:
        drv.record_kernel_events(True)
        try:
            bus = torch.cuda.get_device_properties(local_rank).pci_bus_id
            bus = "%02x:" % int(bus) if isinstance(bus, int) else str(bus)
        except Exception:
            bus = None
        sclk_sampler = SclkSampler(bus)
    with sclk_sampler:
        t0 = time.perf_counter()
        for _ in range(args.steps):
            one_step()
        barrier()
        dt = time.perf_counter() - t0
    sclk, events = None, []
    if args.full:
        drv.record_kernel_events(False)
        sclk = sclk_sampler.summary()
        events = drv.take_kernel_events()
    h2d_per_step = (drv.streamed_bytes() - h2d_before) // max(args.steps, 1)
    if dump_dir and rank == 0:
        dump_outputs(dump_dir, last["results"], merged, K)

    t = torch.tensor([dt], dtype=torch.float64, device=comm_dev)
    if distributed:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt_max = float(t.item())
    gcups = float(sum_q) * total_residues * args.steps / 1e9 / dt_max

    # ---- verification: one more pass, every score of every query (outside the timed region)
    verified, verify_note, cpu_obj = None, None, None
    if not args.no_verify:
        ok = True
        if args.workload == "peak":
            golden = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_scores.json")))["pseudo"].get(str(args.db_length))
            if golden is not None:
                golden = [golden[i] for i in query_index]
            if golden is None:
                ok, verify_note = None, "no golden scores for pseudo-DB length %d" % args.db_length
            else:
                nloc = sum(drv.shard_info(g)["subjects"] for g in range(nshards))
                for qi, q in enumerate(query_letters):
                    drv.scan(q)
                    ids, sc = drv.all_scores()
                    ok = ok and len(sc) == nloc and int(sc.min()) == int(sc.max()) == int(golden[qi])
                    if rank == 0 and K > 0:
                        kk = min(K, total_subjects)
                        base = [r * num for r in range(world)] if not strong else [0]
                        # all scores tie: the K lowest ids win (weak scaling: the replicas' ids are r*num + i)
                        want_ids = sorted(b + i for b in base for i in range(min(kk, num)))[:kk]
                        ok = ok and merged[qi][0].tolist() == [int(golden[qi])] * kk and merged[qi][1].tolist() == want_ids
                verify_note = "all %d scores of every query equal the reference's golden score; merged top-%d scores and ids as expected" % (nloc, K)
        else:
            def top_of_all(sc, ids, k):
                """score desc, id asc — without sorting 6e7 entries: everything at or above the k-th largest score"""
                if k <= 0 or len(sc) == 0:
                    return np.zeros(0, np.int32), np.zeros(0, np.int64)
                kk = min(k, len(sc))
                thr = np.partition(sc, len(sc) - kk)[len(sc) - kk]
                cand = np.nonzero(sc >= thr)[0]
                return search.merge_topk([(sc[cand], ids[cand])], kk)
            big = num > 5_000_000
            gpu_scores = []
            for q in (query_letters if not big else []):
                drv.scan(q)
                ids_all, sc_all = drv.all_scores()
                gpu_scores.append((sc_all, ids_all))
            if want_cpu:
                # the CPU leg scores a seeded sample of the DB (plus the longest subjects): timing AND checker
                chars, offsets, lengths = host_db
                pick, giants = cpu_sample_of(num, args.cpu_sample_subjects or 20000)
                # the timed sample longest subjects first (the ports hand out blocks of consecutive subjects: the long blocks
                # must not be the tail); the longest proteins of the DB are scored for the checker, not timed — four
                # 35 000-residue walks on one thread each made round 5's figure a load-imbalance number, not a rate
                sub = search.build_shard(chars, offsets, lengths, [(int(i), int(i) + 1) for i in pick[::-1]])
                ext = search.build_shard(chars, offsets, lengths, [(int(i), int(i) + 1) for i in giants])
                cpu_obj, cpu_scores = cpu_baseline(queries, sub[0], sub[1], sub[2],
                                                   "%d uniformly sampled subjects (%d residues, longest first) of the same DB; the %d longest subjects scored for the checker, untimed" % (
                                                       len(pick), int(sub[2].astype(np.int64).sum()), len(giants)), extra=ext)
                pick = np.concatenate([pick[::-1], giants])
                for qi in range(len(queries)):
                    if big:     # one query's scores at a time (12 bytes per subject on the host)
                        drv.scan(query_letters[qi])
                        ids, sc = drv.all_scores()
                    else:
                        sc, ids = gpu_scores[qi]
                    by_id = np.empty(num, dtype=np.int32)
                    by_id[ids] = sc     # world == 1: this rank's shards cover every id
                    ok = ok and len(sc) == num and (by_id[pick] == cpu_scores[qi]).all()
                    top = top_of_all(sc, ids, K) if K > 0 else None
                    ok = ok and (K == 0 or (merged[qi][0].tolist() == top[0].tolist() and merged[qi][1].tolist() == top[1].tolist()))
                verify_note = "every score of %d sampled subjects x %d queries equals the CPU oracle; top-%d equals the top of all %d scores" % (
                    len(pick), len(queries), K, num)
            elif big:
                ok, verify_note = None, "not verified: a DB of this size is checked against the CPU leg only (drop --no-cpu-baseline)"
            else:
                # no CPU leg: an independent arithmetic path — all scores again with the int32 kernels only
                d2 = driver.Driver(devices=[local_rank], num_top=0, matrix=62, kinds=(2, 1, 2, 2))
                d2.set_shard(rank, world, 0) if strong else d2.set_shard(0, 1, rank * num)
                d2.db_from_arrays(*host_db)
                d2.upload()
                for qi, q in enumerate(query_letters):
                    d2.scan(q)
                    sc2, ids2 = d2.last_scores(0)
                    o1 = np.argsort(gpu_scores[qi][1], kind="stable")
                    ok = ok and (sc2 == gpu_scores[qi][0][o1]).all() and (ids2 == gpu_scores[qi][1][o1]).all()
                d2.close()
                verify_note = "all scores of every query equal between the %s and the int32 kernel configuration" % kernel_name
        if ok is not None and distributed:
            f = torch.tensor([1 if ok else 0], dtype=torch.int32, device=comm_dev)
            dist.all_reduce(f, op=dist.ReduceOp.MIN)
            ok = bool(f.item())
        verified = None if ok is None else bool(ok)

    if rank == 0:
        cal = device_calibration(local_rank) if events else None
        roof, valu, ktable = roofline_objects(args, workload, kernel_name, events, info, cal, sclk)
        out = {
            "metric": "GCUPS", "value": round(gcups, 2), "unit": "GCUPS", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt_max * 1e3 / args.steps, 3), "higher_is_better": True,
            "scaling": "single" if world == 1 else ("strong" if strong else "weak"), "vs_baseline": None,
            "dtype": DTYPE_BY_KIND[kinds[0]] + (" (int32 results computed in fp32 lanes: exact below 2^24, bound checked per launch)"
                                                if kinds[0] == 2 and os.environ.get("CUDASW4_AMD_I32_NATIVE") != "1" else ""),
            "data": data, "verified": verified, "verified_how": verify_note,
            "config": {"workload": "%s: allqueries.fasta (%d queries, %d residues) vs %s, %s kernel configuration, blosum62, "
                                   "gop -11 gex -1, top %d, C++ host driver" % (args.workload, len(queries), sum_q, what, kernel_name, K),
                       "db_subjects": total_subjects, "db_residues": int(total_residues), "queries": len(queries),
                       "kernel": kernel_name, "host": "libcudasw4_host.so (SearchDriver)",
                       "queries_in_flight": 2 if pipelined else 1,
                       "queries_in_flight_rule": "always two" if pipelined else "two where the driver's rule says so (swdrv_prefers_two_in_flight: %d of the %d queries), else one" % (
                           sum(1 for q in query_letters if drv.prefers_two_in_flight(len(q))), len(query_letters)) if by_rule else "one at a time",
                       # queries of rank 0 whose bulk launch was gated on the dry signal of the query before it (tail
                       # hand-over on small resident shards, include/cudasw4_amd_driver.h: swdrv_tail_overlaps), all steps
                       "tail_overlaps": drv.tail_overlaps(),
                       "numa_node_rank0": env.numa_node, "numa_bound": env.numa_bound,
                       "resident": info["resident"], "residency": residency_of(info),
                       "cached_chars": info.get("cached_chars"), "shard_chars": info["chars"],
                       "shards_on_this_gpu": nshards, "h2d_subject_bytes_per_step": int(h2d_per_step),
                       "parallelism": "db-shard x%d (%s), one top-K gather per step + host merge" % (world, "one DB sharded" if strong else "one DB per rank")},
            "roofline": roof, "valu_roofline": valu,
            # what real data loads a scan with (half2_kernels.cuh:1087-1109, cudasw4.cuh:2134-2172), per step = one pass of
            # the 20 queries over rank 0's shard: subjects whose exact score reached the packed kind's limit (the
            # reference's "num overflows"), subjects the packed kernels flagged and a 32-bit kind re-scored (a few more:
            # the column-offset frame flags early), and the time of the re-score launches (HIP events, inside the timed region)
            "overflow_load": {"num_overflows": load["num_overflows"], "num_rescored": load["num_rescored"],
                              "rescore_launches_per_step": sum(1 for e in events if e.get("rescore")) // max(args.steps, 1) if args.full else None,
                              "rescore_ms_per_step": round(sum(e["ms"] for e in events if e.get("rescore")) / max(args.steps, 1), 3) if args.full else None},
        }
        if not args.full:
            out["verified_how"] = "not checked: a plain run times the steps only (--full verifies every score)"
        if args.kernel_table:
            out["kernels"] = ktable
        if want_cpu and cpu_obj is None:
            # peak workload: a bounded sample of the same DB (identical subjects)
            import oracle_lib as O
            ns = args.cpu_sample_subjects or 40000
            codes = driver.pseudo_sequence(args.db_length, 42)
            sample = O.make_db([codes] * ns)
            cpu_obj, cpu_scores = cpu_baseline(queries, *sample, "%d pseudo subjects of length %d" % (ns, args.db_length))
            if verified and args.workload == "peak":
                golden = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_scores.json")))["pseudo"].get(str(args.db_length))
                if golden is not None and any(int(s[0]) != int(golden[i]) for s, i in zip(cpu_scores, query_index)):
                    out["verified"] = False
        out["cpu_baseline"] = cpu_obj
        if K > 0 and merged[-1] is not None:
            out["config"]["top_merged_example"] = {"query": len(queries) - 1, "scores": merged[-1][0].tolist(),
                                                   "ids": merged[-1][1].tolist()}
    drv.close()
    return out if rank == 0 else None


def main():
    args = parse_args()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # start the ranks BEFORE anything here touches the GPU (a process that has initialised the GPU must not be
        # replaced or forked); the child prints the JSON line
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.stderr.write("bench.py: --gpus %d but WORLD_SIZE=%d; launch with matching values\n" % (args.gpus, world))
        sys.exit(2)
    run_rank(args)


if __name__ == "__main__":
    main()
