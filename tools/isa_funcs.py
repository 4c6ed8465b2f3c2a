#!/usr/bin/env python3
"""Per-function identity of two gfx950 assembly files (tools/isa_diff.sh uses it
for a file whose assembly differs as a whole, e.g. because kernels were added).

    python tools/isa_funcs.py [--allow-missing REGEX] new.s old.s

A function is the text from its `-- Begin function` line to the first text
section directive after its `-- End function` line (its code, its kernel
descriptor, its resource symbols and the compiler's `Kernel info` comment).  Local labels carry the function's index in the file
(.LBB12_3, .Lfunc_end12, and BB12_3 in the loop comments), which shifts when
functions are added or removed before it; the index is taken out before the
comparison, and so is the padding between a label and its comment.  Prints one line per function of
old.s that is missing from new.s or differs, then a summary with the functions
only new.s has.  Exit status 1 when a function of old.s is missing or differs.
--allow-missing names the symbols of an intended removal: a missing function
whose symbol matches REGEX (re.search) is listed as `missing (allowed)` and is
no failure; any other missing function still is.
"""
import hashlib
import re
import sys

BEGIN = re.compile(r"; -- Begin function (\S+)")
LOCAL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI|CPI)\d+")
LOOPS = re.compile(r"\bBB\d+_")  # the same index in the loop comments: `Header=BB12_3`, `Child Loop BB12_7`
# a label's comment is padded to a column: one digit more in the label, one blank less
LABEL = re.compile(r"^(\.L\w+:|; %bb\.\d+:)[ \t]+;")


def normalise(line):
    """The line without its function's index: in the local labels anywhere, in
    the text behind the first `;` (the compiler's comments), and in the
    padding between a label and its comment.  Instruction text is untouched."""
    line = LOCAL.sub(lambda k: ".L" + k.group(1), line)
    line = LABEL.sub(lambda k: k.group(1) + " ;", line)
    code, sep, comment = line.partition(";")
    return code + sep + LOOPS.sub("BB_", comment)


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
                h.update(normalise(line).encode())
    return {k: v.hexdigest() for k, v in out.items()}


def main(argv):
    allowed = None
    if len(argv) == 5 and argv[1] == "--allow-missing":
        allowed, argv = re.compile(argv[2]), argv[:1] + argv[3:]
    if len(argv) != 3:
        raise SystemExit(__doc__)
    new, old = functions(argv[1]), functions(argv[2])
    bad = gone = 0
    for sym, digest in old.items():
        if sym not in new and allowed is not None and allowed.search(sym):
            print(f"  missing (allowed): {sym}")
            gone += 1
        elif sym not in new:
            print(f"  missing: {sym}")
            bad += 1
        elif new[sym] != digest:
            print(f"  differs: {sym}")
            bad += 1
    added = [s for s in new if s not in old]
    print(f"  {len(old) - bad - gone} of {len(old)} existing functions identical, "
          + (f"{gone} missing as allowed, " if allowed is not None else "") + f"{len(added)} added")
    for s in added[:3]:
        print(f"  added: {s}")
    if len(added) > 3:
        print(f"  added: ... and {len(added) - 3} more")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
