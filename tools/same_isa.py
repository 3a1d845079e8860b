#!/usr/bin/env python3
"""Development tool: do two builds hold the same device code?  The gate of a refactoring of the kernel sources.

  tools/same_isa.py A.s B.s        two files of `make asm` (<unit>.gfx950.s)
  tools/same_isa.py A_DIR B_DIR    every *.gfx950.s of either directory, paired by name

One line per kernel symbol: SAME or DIFF and the two instruction counts.  Exit status 1 when a kernel differs or is
missing on either side (or a file, with directories), else 0.

A kernel is the lines between its symbol's label and the end of the function (.Lfunc_end), without comments, blank
lines and assembler directives, and with local labels (.L...) replaced by one token: what is left is the list of its
instructions and their operands.  Text only: no instruction is named or looked for."""
import os
import re
import sys

LOCAL_LABEL = re.compile(r"\.L[A-Za-z0-9_$.]*")


def kernels_of(text):
    """{kernel symbol: [instruction lines]} of one assembly text"""
    lines = text.splitlines()
    symbols = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    out = {}
    for sym in symbols:
        at = next((i for i, l in enumerate(lines) if l.split(";", 1)[0].strip() == sym + ":"), None)
        if at is None:
            continue
        body = []
        for l in lines[at + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            l = l.split(";", 1)[0].strip()              # comments
            if not l or l.startswith("//"):
                continue
            if re.match(r"\.L[A-Za-z0-9_$.]*:$", l) or re.match(r"[A-Za-z_$][\w$.]*:$", l):
                body.append("<label>:")                  # a label of its own line
                continue
            if l.startswith("."):                       # assembler directives
                continue
            body.append(" ".join(LOCAL_LABEL.sub("<label>", l).split()))
        out[sym] = body
    return out


def compare(a_text, b_text, out=sys.stdout, prefix=""):
    """prints the table, returns the number of kernels that differ or are missing on one side"""
    a, b = kernels_of(a_text), kernels_of(b_text)
    bad = 0
    for sym in sorted(set(a) | set(b)):
        if sym not in a or sym not in b:
            bad += 1
            out.write("%sMISSING %6s %6s  %s\n" % (prefix, len(a[sym]) if sym in a else "-", len(b[sym]) if sym in b else "-", sym))
            continue
        same = a[sym] == b[sym]
        bad += not same
        out.write("%s%s %6d %6d  %s\n" % (prefix, "SAME" if same else "DIFF", len(a[sym]), len(b[sym]), sym))
    if not a and not b:
        out.write("%sno kernel in either text\n" % prefix)
        bad += 1
    return bad


def main(argv):
    if len(argv) != 3:
        sys.stderr.write(__doc__)
        return 2
    a, b = argv[1], argv[2]
    if os.path.isdir(a) != os.path.isdir(b):
        sys.stderr.write("same_isa: two files or two directories\n")
        return 2
    if not os.path.isdir(a):
        return 1 if compare(open(a).read(), open(b).read()) else 0
    units = lambda d: set(f for f in os.listdir(d) if f.endswith(".gfx950.s"))
    bad = 0
    for f in sorted(units(a) | units(b)):
        if f not in units(a) or f not in units(b):
            print("MISSING file %s (in %s only)" % (f, "A" if f in units(a) else "B"))
            bad += 1
            continue
        print(f)
        bad += compare(open(os.path.join(a, f)).read(), open(os.path.join(b, f)).read(), prefix="  ")
    print("%d kernel(s) differ or are missing" % bad if bad else "all kernels SAME")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
