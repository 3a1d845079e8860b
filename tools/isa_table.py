#!/usr/bin/env python3
"""Development tool: per-kernel register, scratch, spill, static LDS and instruction counts of `make asm` output, and the difference
between two builds.

  tools/isa_table.py DIR                  one table: the *.gfx950.s files of DIR
  tools/isa_table.py BEFORE_DIR DIR       the same with the change since BEFORE_DIR per column

Kernels are named by a regular expression on the demangled-looking part of the symbol (--match, default: the ray-batch
kernels closest / occluded / shade / view); registers and scratch come from the .amdgpu_metadata block, instructions are
counted between the kernel's label and its .Lfunc_end."""
import argparse
import glob
import os
import re

FIELDS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")
HEAD = ("VGPR", "SGPR", "scratch", "vspill", "sspill", "LDS", "insts")       # LDS: the static part, bytes


def kernels_of(path):
    text = open(path).read()
    out = {}
    for block in re.split(r"\n  - \.agpr_count:", text.split(".amdgpu_metadata", 1)[1])[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = [int(re.search(r"\.%s:\s+(\d+)" % f, block).group(1)) for f in FIELDS]
    for name in out:
        body = re.split(r"\n%s:[^\n]*\n" % re.escape(name), text, 1)[1].split(".Lfunc_end", 1)[0]
        out[name].append(sum(1 for l in body.splitlines() if re.match(r"\s+[a-z]\w*(\s|$)", l)))
    return out


def table(directory, match):
    rows = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.gfx950.s"))):
        for name, v in kernels_of(path).items():
            if re.search(match, name):
                rows[name] = v
    return rows


def short(name):
    m = re.match(r"_ZN\d+(rtx\w?)\d+(\w+_kernel)ILb([01])ELb([01])EEv", name)      # the kernels with exactly these two parameters
    return "%s::%s<COUNT=%s, SPHERES=%s>" % m.groups() if m else name


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dirs", nargs="+")
    ap.add_argument("--match", default=r"(closest|occluded|shade|view)_kernelILb")
    a = ap.parse_args()
    after = table(a.dirs[-1], a.match)
    before = table(a.dirs[0], a.match) if len(a.dirs) == 2 else None
    print("%-56s" % "kernel" + "".join("%16s" % h for h in HEAD))
    for name in sorted(after, key=short):
        cells = []
        for k, v in enumerate(after[name]):
            if before is None:
                cells.append("%d" % v)
            else:
                cells.append("%d (%+d)" % (v, v - before[name][k]) if name in before else "%d (new)" % v)
        print("%-56s" % short(name) + "".join("%16s" % c for c in cells))
    if before is not None:
        for name in sorted(set(before) - set(after), key=short):
            print("%-48s  gone" % short(name))


if __name__ == "__main__":
    main()
