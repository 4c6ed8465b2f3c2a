#!/usr/bin/env python3
"""Per-function identity of two gfx950 assembly files (tools/isa_diff.sh uses it
for a file whose assembly differs as a whole, e.g. because kernels were added).

    python tools/isa_funcs.py new.s old.s

A function is the text from its `-- Begin function` line to the first text
section directive after its `-- End function` line (its code, its kernel
descriptor, its resource symbols and the compiler's `Kernel info` comment).  Local labels carry the function's index in the file
(.LBB12_3, .Lfunc_end12), which shifts when functions are added before it; the
index is taken out before the comparison.  Prints one line per function of
old.s that is missing from new.s or differs, then a summary with the functions
only new.s has.  Exit status 1 when a function of old.s is missing or differs.
"""
import hashlib
import re
import sys

BEGIN = re.compile(r"; -- Begin function (\S+)")
LOCAL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI|CPI)\d+")


def functions(path):
    """{symbol: sha256 of its normalised text}, in file order."""
    out, name, h, ended = {}, None, None, False
    with open(path, errors="replace") as f:
        for line in f:
            m = BEGIN.search(line)
            if m:
                name, h, ended = m.group(1), hashlib.sha256(), False
                out[name] = h
            elif name is not None and "; -- End function" in line:
                ended = True
            elif ended and (line.startswith("\t.text") or line.startswith("\t.section\t.text")):
                name = None  # back in a text section: the next function's, or the file's epilogue
            if name is not None:
                h.update(LOCAL.sub(lambda k: ".L" + k.group(1), line).encode())
    return {k: v.hexdigest() for k, v in out.items()}


def main(argv):
    if len(argv) != 3:
        raise SystemExit(__doc__)
    new, old = functions(argv[1]), functions(argv[2])
    bad = 0
    for sym, digest in old.items():
        if sym not in new:
            print(f"  missing: {sym}")
            bad += 1
        elif new[sym] != digest:
            print(f"  differs: {sym}")
            bad += 1
    added = [s for s in new if s not in old]
    print(f"  {len(old) - bad} of {len(old)} existing functions identical, {len(added)} added")
    for s in added[:3]:
        print(f"  added: {s}")
    if len(added) > 3:
        print(f"  added: ... and {len(added) - 3} more")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
