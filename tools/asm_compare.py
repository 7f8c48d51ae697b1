#!/usr/bin/env python3
"""Compares the device assembly of two builds kernel by kernel: which kernels keep their mangled name and their instruction stream.

    make -C everglades-ai-wargame_amd/csrc asm            (writes /tmp/evg_kernels.s; do it in both trees and keep the two files)
    python tools/asm_compare.py PARENT.s NEW.s            (section 3 of profiles/r11_a_minimized_isa.txt)

Instructions only: comments, assembler directives and the numbering of local labels are dropped.  Exit status 1 if a kernel of the first file is missing
from the second or has another instruction stream."""
import re
import sys


def kernels(path):
    out, name, lines = {}, None, None
    for l in open(path):
        m = re.match(r"^(_Z\w+):", l)
        if m and name is None:
            name, lines = m.group(1), []
            continue
        if name is not None:
            if l.startswith(".Lfunc_end"):
                out[name], name = lines, None
                continue
            c = l.split(";")[0].rstrip()
            if c.strip() and not c.strip().startswith("."):
                lines.append(re.sub(r"\.LBB\d+_", ".LBB_", c))
    return out


def main(parent, new):
    a, b = kernels(parent), kernels(new)
    same = [n for n in a if n in b and a[n] == b[n]]
    diff = [n for n in a if n in b and a[n] != b[n]]
    gone = [n for n in a if n not in b]
    added = [n for n in b if n not in a]
    print("kernels in the parent: %d; same mangled name and identical instruction stream in this build: %d; different: %d; missing: %d; new: %d" % (
        len(a), len(same), len(diff), len(gone), len(added)))
    print()
    for n in sorted(a):
        print("%-5s %6d instructions  %s" % ("same" if n in same else ("DIFF" if n in diff else "GONE"), len(a[n]), n))
    print()
    for n in sorted(added):
        print("%-5s %6d instructions  %s" % ("new", len(b[n]), n))
    return 1 if diff or gone else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
