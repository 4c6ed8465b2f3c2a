#!/bin/bash
# Device-code identity of the working tree against a git revision (no GPU
# needed): the gate of a refactor that must not change an instruction.
#   tools/isa_diff.sh <git-rev>
# Each .hip file that <git-rev> has too is compiled to gfx950 assembly with the
# Makefile's HIPFLAGS, once from the working tree and once from a temporary
# git worktree of <rev> (removed afterwards), and the two .s files are
# compared byte for byte.  Both sides get the same -cuid=: by default hipcc
# derives the compilation-unit id (the __hip_cuid_* symbol) from the source
# path, the only path-dependent text in the assembly.  One line per
# file: identical (with the sha256 of the .s), or the symbol that holds the
# first difference; a file the revision lacks is reported as new.  A file that
# differs as a whole is compared function by function (tools/isa_funcs.py): when
# every function of <git-rev> is there unchanged, functions were only added,
# which is reported and is no difference.  Exit status 1 on any difference.
# rt_kernel.hip takes minutes per compile; the compiles run ISA_JOBS (default
# 4) at a time.  Two optional variables, for a refactor that runs the gate
# once per step:
#   ISA_OLD_DIR=<dir>        keep the revision's .s files in
#                            <dir>/<commit sha>-<hash of the compile command>/
#                            and reuse the ones already there, so <git-rev> is
#                            compiled once per set of flags and not on every run
#   ISA_ALLOW_MISSING=<re>   functions of <git-rev> whose symbol matches <re>
#                            may be missing (an intended removal); any other
#                            missing function is still a difference
set -eu
[ $# -eq 1 ] || { echo "usage: $0 <git-rev>" >&2; exit 2; }
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap 'git -C "$R" worktree remove --force "$T/rev" >/dev/null 2>&1 || true; rm -rf "$T"' EXIT
git -C "$R" worktree add --detach "$T/rev" "$1" >/dev/null
CC=$(make -s -C "$R" --eval 'isa-cc: ; @echo $(HIPCC) $(HIPFLAGS)' isa-cc)
OLD="$T/old"
[ -z "${ISA_OLD_DIR:-}" ] ||
    OLD="$(mkdir -p "$ISA_OLD_DIR" && cd "$ISA_OLD_DIR" && pwd)/$(git -C "$T/rev" rev-parse HEAD)-$(echo "$CC" | sha256sum | cut -c1-12)"
FILES="rt_kernel rt_mis rt_rays rt_lbvh rt_gsah rt_refit rt_aov rt_denoise rt_reproject rt_adaptive rt_mathcheck"
mkdir -p "$T/new" "$OLD"
export CC T
for f in $FILES; do
    echo "$T/new $f $R"
    [ -f "$OLD/$f.s" ] || echo "$OLD $f $T/rev"
done | xargs -P "${ISA_JOBS:-4}" -L 1 bash -c \
    'cd "$3" && { [ -f gpuraytracer_amd/csrc/$2.hip ] || exit 0; } && $CC --offload-device-only -S -cuid=isa_diff gpuraytracer_amd/csrc/$2.hip -o "$1/$2.s.tmp" 2>"$T/$2.$$.err" &&
         mv "$1/$2.s.tmp" "$1/$2.s" || { cat "$T/$2.$$.err" >&2; exit 255; }' _
rc=0
for f in $FILES; do
    if [ ! -f "$OLD/$f.s" ]; then  # a file <git-rev> does not have: nothing to compare
        echo "$f.hip: new (sha256 $(sha256sum <"$T/new/$f.s" | cut -d' ' -f1))"
    elif cmp -s "$T/new/$f.s" "$OLD/$f.s"; then
        echo "$f.hip: identical (sha256 $(sha256sum <"$T/new/$f.s" | cut -d' ' -f1))"
    elif funcs=$(python3 "$R/tools/isa_funcs.py" ${ISA_ALLOW_MISSING:+--allow-missing "$ISA_ALLOW_MISSING"} "$T/new/$f.s" "$OLD/$f.s"); then
        # the file as a whole differs, but every function <git-rev> has is identical (or allowed to be missing)
        echo "$f.hip: existing functions identical; functions added or allowed to be missing"
        echo "$funcs"
    else
        # the last symbol label (name: in column 0, not a local .L label) at or before the first differing line
        line=$(cmp "$T/new/$f.s" "$OLD/$f.s" | sed -n 's/.* line \([0-9]*\)$/\1/p')
        sym=$(head -n "${line:-1}" "$T/new/$f.s" | grep -E '^[A-Za-z_$][A-Za-z0-9_.$]*:' | tail -1)
        echo "$f.hip: DIFFERS at line ${line:-?} of the assembly, in ${sym%:}"
        echo "$funcs"
        rc=1
    fi
done
exit $rc
