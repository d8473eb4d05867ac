#!/bin/bash
# Is the DEVICE code of a file of accv-lab_amd/csrc (default draw_heatmap.hip) the same as at an earlier commit (default HEAD)?  Compiles the file
# of that commit (exported into build/asm_cmp/prev, like build_prev_lib.sh) and of the working tree to gfx950 assembly with
# the Makefile's flags and diffs the two, less the lines that carry the per-compilation __hip_cuid_<hash> symbol (the only
# lines in which two compilations of one source differ).  An empty diff = all kernels, their metadata and their order are
# byte-identical: a source-only refactor has the speed of its parent.  Exit status 1 when the assembly differs.
#   scripts/compare_device_asm.sh [REV] [FILE.hip] [-DFOO ...]      extra switches go to both compilations (-DACCV_SPLAT_STAMPS)
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
REV="HEAD"
SRC="draw_heatmap.hip"
if [ $# -gt 0 ] && [ "${1#-}" = "$1" ] && [ "${1%.hip}" = "$1" ]; then REV="$1"; shift; fi
if [ $# -gt 0 ] && [ "${1%.hip}" != "$1" ]; then SRC="$1"; shift; fi
OUT="$ROOT/build/asm_cmp"
rm -rf "$OUT" && mkdir -p "$OUT/prev"
git -C "$ROOT" archive "$REV" accv-lab_amd/csrc include | tar -x -C "$OUT/prev"
FLAGS=(-O3 -std=c++17 -fPIC --offload-arch=gfx950 -I../../include -I. -Wall -Wno-unused-function -fno-gpu-rdc -pthread
       --cuda-device-only -S "$@")
echo "revision: $(git -C "$ROOT" rev-parse --short "$REV") against the working tree"
echo "command:  (in accv-lab_amd/csrc) hipcc ${FLAGS[*]} $SRC -o <out>.s"
(cd "$OUT/prev/accv-lab_amd/csrc" && /opt/rocm/bin/hipcc "${FLAGS[@]}" "$SRC" -o "$OUT/prev.s")
(cd "$ROOT/accv-lab_amd/csrc" && /opt/rocm/bin/hipcc "${FLAGS[@]}" "$SRC" -o "$OUT/new.s")
grep -v __hip_cuid_ "$OUT/prev.s" > "$OUT/prev.nocuid.s"
grep -v __hip_cuid_ "$OUT/new.s" > "$OUT/new.nocuid.s"
echo "lines:    $(wc -l < "$OUT/prev.s") at the revision, $(wc -l < "$OUT/new.s") in the working tree"
echo "kernels:  $(grep -c '^[[:space:]]*\.amdhsa_kernel ' "$OUT/prev.s") at the revision, $(grep -c '^[[:space:]]*\.amdhsa_kernel ' "$OUT/new.s") in the working tree"
echo "compiler: $(grep -m1 '\.ident' "$OUT/new.s" | sed 's/^[[:space:]]*//')"
echo "diff prev.nocuid.s new.nocuid.s:"
if diff "$OUT/prev.nocuid.s" "$OUT/new.nocuid.s" > "$OUT/asm.diff"; then
  echo "(empty) device assembly identical"
else
  # which kernels the differing lines belong to (the .s lists each function under its mangled name as a label)
  echo "$(grep -c '^[<>]' "$OUT/asm.diff") differing lines, full diff in build/asm_cmp/asm.diff; by function, counted in the working tree's file:"
  diff --unchanged-line-format= --old-line-format= --new-line-format='%dn
' "$OUT/prev.nocuid.s" "$OUT/new.nocuid.s" > "$OUT/changed_lines.txt" || true
  awk 'NR==FNR { changed[$1] = 1; next }
       /^_Z[A-Za-z0-9_]*:/ { fn = $1 }
       (FNR in changed) { n[fn]++ }
       END { for (f in n) print n[f], f }' "$OUT/changed_lines.txt" "$OUT/new.nocuid.s" | sort -rn | while read -r cnt name; do
    echo "  $cnt  $(echo "${name%:}" | { c++filt 2>/dev/null || cat; })"
  done
  exit 1
fi
