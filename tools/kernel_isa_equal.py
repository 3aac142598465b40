#!/usr/bin/env python3
"""Are the kernels of two builds the same machine code?  (no GPU needed)
python tools/kernel_isa_equal.py PARENT_DIR CHILD_DIR
Each directory holds the .s files of `make -C functracer_amd/csrc device-asm` (hipcc -S --cuda-device-only): the parent commit's, built in a
checkout of its own, and this tree's.  Every kernel of the parent must be in the child, with the same body and the same .amdhsa_ descriptor
lines, once comments are stripped and local labels (.LBB<n>_<m>, .Lpost_getpc<n>, any .L...) are renumbered in order of appearance: their
numbers count the functions and blocks of the whole unit, not of the kernel.  Text is compared for equality and nothing else.  One line
per kernel; the exit status is 0 when all are equal."""
import glob
import os
import re
import subprocess
import sys


def kernels_of(directory):
    found = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = [ln.split(";", 1)[0].strip() for ln in open(path)]
        lines = [ln for ln in lines if ln]
        start = {ln[:-1]: k for k, ln in enumerate(lines) if ln.endswith(":") and not ln.startswith(".")}
        for k, ln in enumerate(lines):
            if not ln.startswith(".amdhsa_kernel "):
                continue
            name = ln.split()[1]
            end = next(e for e in range(k, len(lines)) if lines[e] == ".end_amdhsa_kernel")
            body_end = next(e for e in range(start[name], len(lines)) if lines[e].startswith(".Lfunc_end"))
            labels = {}
            text = "\n".join(lines[start[name]:body_end] + lines[k:end])
            found[name] = re.sub(r"\.L[A-Za-z_$.]*\d[\w$.]*", lambda m: labels.setdefault(m.group(0), f".L#{len(labels)}"), text)
    return found


parent, child = kernels_of(sys.argv[1]), kernels_of(sys.argv[2])
names = sorted(set(parent) | set(child))
plain = dict(zip(names, subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines())) if names else {}
bad = 0
for name in names:
    if name not in parent:
        verdict = "new"                                             # (not an error: the parent has nothing to compare it with)
    elif name not in child:
        verdict = "MISSING"
    else:
        verdict = "equal" if parent[name] == child[name] else "DIFFERENT"
    bad += verdict in ("MISSING", "DIFFERENT")
    size = (child.get(name) or parent[name]).count("\n") + 1
    print(f"{verdict:9s} {size:6d} lines  {re.sub(r'ftk::.anonymous namespace.::|^void ', '', plain[name]).split('(')[0]}")
print(f"{len(parent)} kernels in {sys.argv[1]}, {len(child)} in {sys.argv[2]}: " + ("all equal" if not bad else f"{bad} missing or different"))
sys.exit(1 if bad else 0)
