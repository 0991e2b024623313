#!/usr/bin/env python3
"""Are two builds the same device code?  Compares the gfx950 code objects of every object file that two object
directories have in common (no GPU needed):

    python tools/isa_diff.py OLD_OBJ_DIR NEW_OBJ_DIR [name.o ...]

Per translation unit it prints the symbols that only one side has, the symbols whose disassembly differs (with the
number of differing lines) and the kernels whose code-object metadata differs.  Exit status 0: no difference at all.
The comparison is for equality only; nothing in the text is interpreted."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META_KEYS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
             "private_segment_fixed_size")


def tool(name, *args):
    return subprocess.check_output([os.path.join(LLVM, name)] + list(args), text=True, stderr=subprocess.DEVNULL)


def code_object(obj, td):
    """The gfx950 code object inside a host object file (as tools/kernel_regs.py extracts it)."""
    co, fb = os.path.join(td, "k.co"), os.path.join(td, "k.fatbin")
    try:
        tool("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, obj)
    except subprocess.CalledProcessError:
        return None   # a translation unit without device code
    tool("clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fb, "--output=" + co)
    return co


def disassembly(co):
    """symbol -> its lines, without the addresses (a symbol keeps its text when its neighbours move)"""
    syms, cur = {}, None
    for line in tool("llvm-objdump", "-d", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = syms.setdefault(m.group(1), [])
        elif cur is not None and line.strip() and line.strip() != "...":   # ("...": zero padding behind the last symbol)
            cur.append(re.sub(r"//\s*[0-9A-Fa-f]+:", "//", line).strip())
    return syms


def metadata(co):
    """kernel name -> {key: value} of its entry in the code object's notes"""
    out = {}
    for block in tool("llvm-readelf", "--notes", co).split("- .agpr_count")[1:]:
        fields = dict(re.findall(r"^\s+\.(\w+):\s+(\S+)\s*$", ".agpr_count" + block, flags=re.M))
        if "name" in fields:
            out[fields["name"]] = fields
    return out


def describe(obj):
    with tempfile.TemporaryDirectory() as td:
        co = code_object(obj, td)
        return (disassembly(co), metadata(co)) if co else ({}, {})


def compare(name, old, new):
    """prints the differences of one translation unit; returns their number"""
    (otext, ometa), (ntext, nmeta) = describe(old), describe(new)
    found = 0
    for side, a, b in (("old", otext, ntext), ("new", ntext, otext)):
        for sym in sorted(set(a) - set(b)):
            print("%s: only in %s: %s" % (name, side, sym))
            found += 1
    for sym in sorted(set(otext) & set(ntext)):
        if otext[sym] != ntext[sym]:
            lines = sum(1 for d in difflib.ndiff(otext[sym], ntext[sym]) if d[:1] in "+-")
            print("%s: text differs (%d lines; %d -> %d): %s" % (name, lines, len(otext[sym]), len(ntext[sym]), sym))
            found += 1
    for sym in sorted(set(ometa) & set(nmeta)):
        keys = [k for k in sorted(set(ometa[sym]) | set(nmeta[sym])) if ometa[sym].get(k) != nmeta[sym].get(k)]
        if keys:
            print("%s: metadata differs: %s: %s" % (name, sym, ", ".join(
                "%s %s -> %s" % (k, ometa[sym].get(k), nmeta[sym].get(k)) for k in sorted(keys, key=lambda k: k not in META_KEYS))))
            found += 1
    for side, a, b in (("old", ometa, nmeta), ("new", nmeta, ometa)):
        for sym in sorted(set(a) - set(b)):
            print("%s: kernel metadata only in %s: %s" % (name, side, sym))
            found += 1
    print("%s: %d symbols, %d kernels, %s" % (name, len(ntext), len(nmeta), "identical" if not found else "%d differences" % found))
    return found


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    old_dir, new_dir, only = argv[1], argv[2], argv[3:]
    objs = lambda d: {f for f in os.listdir(d) if f.endswith(".o")}
    found = 0
    for side, a, b in ((old_dir, objs(old_dir), objs(new_dir)), (new_dir, objs(new_dir), objs(old_dir))):
        for f in sorted(a - b):
            if not only or f in only:
                print("%s: only in %s" % (f, side))
                found += 1
    for f in sorted(objs(old_dir) & objs(new_dir)):
        if not only or f in only:
            found += compare(f, os.path.join(old_dir, f), os.path.join(new_dir, f))
    print("isa_diff: %s" % ("no difference" if not found else "%d differences" % found))
    return 1 if found else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
