#!/usr/bin/env python3
"""Static VALU census of the packed scan kernels: VALU instructions per quad (four anti-diagonal steps) of the main quad loop
of sw_scan_kernel, and per cell pair (quad / (4 R)), next to its scratch accesses and the code object's register counts.

    python tools/valu_census.py                   # compile the packed 16-lane multi-stripe kernels of R = 25..32 and report
    python tools/valu_census.py --rows 32 --lanes 16 --single
    python tools/valu_census.py file.s            # report on an assembly file (hipcc -S --cuda-device-only)

The main loop is the leanest innermost loop that runs whole quads (tools/loop_spills.py finds the loops)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_spills as LS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudasw4_amd", "csrc")
KINDS = {"0": "F16X2", "1": "I16X2", "2": "I32", "3": "F32"}


def report(path):
    text = open(path).read().split("\n")
    # the code-object metadata behind the kernels: .vgpr_count / .vgpr_spill_count / .sgpr_spill_count per kernel name
    regs = {}
    cur = None
    for l in text:
        m = re.match(r"\s+\.name:\s+(\S+)", l)
        if m:
            cur = m.group(1)
        for key in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count"):
            m = re.match(r"\s+\.%s:\s+(\d+)" % key, l)
            if m and cur:
                regs.setdefault(cur, {})[key] = int(m.group(1))
    rows = []
    for name, lines in LS.kernels(path):
        m = re.search(r"sw_scan_kernelILi(\d)ELi(\d+)ELi(\d+)ELb(\d)ELb(\d)E", name)
        if not m:
            continue
        kind, R, lanes, multi, offs = m.groups()
        loops = LS.loops(lines)
        inner = [(a, b) for a, b in loops if not any(a < c and d < b for c, d in loops)]
        best = None
        for a, b in inner:
            body = lines[a:b + 1]
            valu = sum(1 for l in body if re.match(r"\s+v_", l))
            scratch = sum(1 for l in body if re.match(r"\s+scratch_", l))
            maxes = sum(1 for l in body if re.match(r"\s+v_(pk_maximum3|max3)", l))
            # a loop over whole quads (at least two 3-input maxima per row and step); the leanest such copy of the body
            # (a kernel may keep more than one, e.g. for quads that lower the frame)
            if maxes >= 8 * int(R) and (best is None or valu < best[0]):
                best = (valu, scratch)
        if best is None:
            continue
        r = regs.get(name, {})
        rows.append((KINDS[kind], int(R), int(lanes), multi == "1", best[0], best[0] / (4.0 * int(R)), best[1],
                     r.get("vgpr_count"), r.get("vgpr_spill_count"), r.get("sgpr_spill_count")))
    print("%-6s %3s %5s %5s %10s %14s %12s %5s %11s %11s" % ("kind", "R", "lanes", "multi", "VALU/quad", "VALU/cellpair",
                                                            "loop scratch", "VGPRs", "VGPR spills", "SGPR spills"))
    for k in sorted(rows, key=lambda x: (x[0], x[2], x[3], x[1])):
        print("%-6s %3d %5d %5s %10d %14.3f %12d %5s %11s %11s" % k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm", nargs="?", help="an assembly file; default: compile the selected kernels")
    ap.add_argument("--rows", default="25-32", help="R or a range lo-hi")
    ap.add_argument("--lanes", type=int, default=16)
    ap.add_argument("--single", action="store_true", help="single-stripe kernels instead of multi-stripe ones")
    args = ap.parse_args()
    if args.asm:
        report(args.asm)
        return
    lo, _, hi = args.rows.partition("-")
    rs = range(int(lo), int(hi or lo) + 1)
    multi = "false" if args.single else "true"
    src = '#include "sw_launch.hpp"\nnamespace swk {\n' + "".join(
        "template __global__ void sw_scan_kernel<%s, %d, %d, %s, true>(const ScanParams);\n" % (k, r, args.lanes, multi)
        for k in ("F16X2", "I16X2") for r in rs) + "}\n"
    with tempfile.TemporaryDirectory() as d:
        hip, asm = os.path.join(d, "census.hip"), os.path.join(d, "census.s")
        open(hip, "w").write(src)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                               "-I", CSRC, hip, "-o", asm], stderr=subprocess.DEVNULL)
        report(asm)


if __name__ == "__main__":
    main()
