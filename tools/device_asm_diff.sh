#!/bin/bash
# device_asm_diff.sh [base-rev] -- proves that a host-side change left the device code alone.
# Compiles every file of the Makefile's SRCS with its FLAGS plus --cuda-device-only -S, once from <base-rev> (default HEAD,
# taken with git archive) and once from the working tree, drops the lines that depend on the source text and not on the kernels
# (.file, .ident, the __hip_cuid_ hash of the translation unit) and compares file by file.  No GPU needed.
# Exit status 0: every file identical.  JOBS=<n> compiles in parallel (default 8); KEEP=<dir> keeps the assembly there.
set -euo pipefail
base=${1:-HEAD}
root=$(git -C "$(dirname "$0")" rev-parse --show-toplevel)
work=${KEEP:-$(mktemp -d)}
mkdir -p "$work/base" "$work/asm_base" "$work/asm_tree"
[ -n "${KEEP:-}" ] || trap 'rm -rf "$work"' EXIT
git -C "$root" archive "$base" cvt_amd/csrc include | tar -x -C "$work/base"

mk="$root/cvt_amd/csrc/Makefile"
hipcc=${HIPCC:-/opt/rocm/bin/hipcc}
flags=$(make -s -f "$mk" --eval 'pf: ; @echo $(FLAGS)' pf)
srcs=$(make -s -f "$mk" --eval 'ps: ; @echo $(SRCS)' ps)

emit() {  # <source dir> <output dir>: skips files already there (KEEP=)
    local src=$1 out=$2 f
    for f in $srcs; do [ -s "$out/${f%.hip}.s" ] || echo "$f"; done |
        xargs -r -P "${JOBS:-8}" -I{} sh -c \
            "$hipcc $flags --cuda-device-only -S '$src/{}' -o '$out/{}.raw' 2>'$out/{}.log' && grep -v -e '^[[:space:]]*\.file' -e '^[[:space:]]*\.ident' -e '__hip_cuid_' '$out/{}.raw' > '$out/{}.tmp' && rm '$out/{}.raw'"
    for f in $srcs; do [ -e "$out/$f.tmp" ] && mv "$out/$f.tmp" "$out/${f%.hip}.s"; done
    return 0
}
emit "$work/base/cvt_amd/csrc" "$work/asm_base"
emit "$root/cvt_amd/csrc" "$work/asm_tree"

bad=0
for f in $srcs; do
    s=${f%.hip}.s
    if cmp -s "$work/asm_base/$s" "$work/asm_tree/$s"; then echo "identical  $f"; else echo "DIFFERS    $f"; bad=$((bad + 1)); fi
done
echo "$bad of $(echo $srcs | wc -w) files differ from $base"
[ "$bad" -eq 0 ]
