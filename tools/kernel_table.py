#!/usr/bin/env python3
"""Per-kernel static table of a device-only assembly listing, or of two side by side.

  hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S -o head.s csrc/pt_render.hip
  tools/kernel_table.py parent.s head.s > kernel_table.txt

Per kernel: instruction count (the lines between the kernel's label and its descriptor that are neither
labels, directives nor comments), VGPRs, SGPRs, scratch bytes per lane and static LDS bytes per workgroup,
from the compiler's "Kernel info" block.  With two listings every kernel gets one row, and a row whose
resource figures differ is marked with '*'.
"""
import re
import subprocess
import sys

INFO = {"TotalNumSgprs": "sgpr", "NumVgprs": "vgpr", "ScratchSize": "scratch", "LDSByteSize": "lds"}


def parse(path):
    kernels, order = {}, []
    name, count, cur = None, 0, None
    with open(path, errors="replace") as f:
        lines = f.readlines()
    for line in lines:
        m = re.match(r"(\w+):\s*; @\1", line)
        if m:
            name, count = m.group(1), 0
            continue
        if name:
            if line.startswith("\t.section") or line.startswith("\t.amdhsa_kernel"):
                cur = kernels[name] = {"insts": count}
                order.append(name)
                name = None
            elif line.startswith("\t") and not line.lstrip().startswith((".", ";")):
                count += 1
            continue
        m = re.match(r"; (\w+):? (?:= )?(\d+)", line)
        if m and cur is not None and m.group(1) in INFO:
            cur[INFO[m.group(1)]] = int(m.group(2))
    return kernels, order


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"^void |\(KParams\)$", "", d.replace("(anonymous namespace)::", "")) for n, d in zip(names, out)}


COLS = ("insts", "vgpr", "sgpr", "scratch", "lds")


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit("usage: kernel_table.py LISTING.s [HEAD_LISTING.s]")
    tables = [parse(p) for p in sys.argv[1:3]]
    names = tables[0][1] + [n for t in tables[1:] for n in t[1] if n not in tables[0][0]]
    pretty = demangle(names)
    two = len(tables) == 2
    print("# " + ("parent -> head: " if two else "") + " ".join(COLS) + "  kernel   (* = a resource figure differs)")
    changed = 0
    for n in names:
        rows = [t[0].get(n) for t in tables]
        cells = []
        for c in COLS:
            v = [str(r[c]) if r else "-" for r in rows]
            cells.append(v[0] if len(set(v)) == 1 else "->".join(v))
        diff = two and any((rows[0] or {}).get(c) != (rows[1] or {}).get(c) for c in COLS[1:])
        changed += diff
        print("%s %-11s %-7s %-9s %-7s %-6s %s" % ("*" if diff else " ", *cells, pretty[n]))
    if two:
        print("# %d kernels, %d with a changed resource figure" % (len(names), changed))


if __name__ == "__main__":
    main()
