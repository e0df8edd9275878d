#!/bin/bash
# device_asm_diff.sh [base-rev] -- proves that a host-side change, or a refactoring of device code, left the kernels alone.
# Compiles every file of the Makefile's SRCS with its FLAGS plus --cuda-device-only -S, once from <base-rev> (default HEAD,
# taken with git archive) and once from the working tree, drops the lines that depend on the source text and not on the kernels
# (.file, .ident, the __hip_cuid_ hash of the translation unit) and compares file by file.  For a file that differs it lists the
# functions (kernels and non-inlined device functions) whose instruction stream or kernel descriptor differs, with the number of
# changed lines and whether the descriptor's registers / LDS / scratch moved.  No GPU needed.
# Exit status 0: every file identical.  JOBS=<n> compiles in parallel (default 8); KEEP=<dir> keeps the assembly there
# (and reuses what is there: delete <dir>/asm_tree/<file>.s to compile a file again).  RENAME=<sed script> is applied to the base's
# assembly first: for a change that renames a type or function which appears in mangled names (every reference would differ).
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
filt=$(command -v llvm-cxxfilt || command -v c++filt || echo cat)

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

# one file per function under <dir>: its body (.type ... @function to .Lfunc_end) and, for a kernel, its .amdhsa_kernel descriptor
split_fns() {  # <file.s> <dir>
    rm -rf "$2"; mkdir -p "$2"
    awk -v out="$2" '
        function path(n) { return out "/" (length(n) < 200 ? n : substr(n, 1, 180) "_" length(n)) }
        /^[[:space:]]*\.type[[:space:]].*,@function/ { n = $2; sub(/,@function.*/, "", n); cur = path(n) }
        /^[[:space:]]*\.amdhsa_kernel[[:space:]]/ { cur = path($2) }
        cur != "" { print >> cur }
        /^\.Lfunc_end/ || /^[[:space:]]*\.end_amdhsa_kernel/ { close(cur); cur = "" }
    ' "$1"
}
res='amdhsa_next_free_[vs]gpr|amdhsa_accum_offset|amdhsa_group_segment_fixed_size|amdhsa_private_segment_fixed_size'
by_function() {  # <file.s name>
    local b="$work/fn_base/${1%.s}" t="$work/fn_tree/${1%.s}" n lines moved shown=0
    split_fns "$work_base/$1" "$b"
    split_fns "$work/asm_tree/$1" "$t"
    for n in $( (ls "$b"; ls "$t") | sort -u); do
        if [ ! -e "$b/$n" ]; then echo "    new      $(echo "$n" | $filt)"; shown=1; continue; fi
        if [ ! -e "$t/$n" ]; then echo "    gone     $(echo "$n" | $filt)"; shown=1; continue; fi
        cmp -s "$b/$n" "$t/$n" && continue
        lines=$(diff "$b/$n" "$t/$n" | grep -c '^[<>]' || true)
        moved=$(diff "$b/$n" "$t/$n" | grep -E "^[<>].*($res)" | tr -s '[:space:]' ' ' | tr '\n' ';' || true)
        echo "    $(printf '%6d' "$lines") lines  $(echo "$n" | $filt)  resources: ${moved:-same}"
        shown=1
    done
    [ "$shown" -eq 1 ] || echo "    (every function identical: the difference lies in data or metadata outside them)"
}

if [ -n "${RENAME:-}" ]; then  # the change renames a type or function: bring the base's (mangled) symbol names along
    mkdir -p "$work/asm_base_renamed"
    for f in $srcs; do sed -e "$RENAME" "$work/asm_base/${f%.hip}.s" > "$work/asm_base_renamed/${f%.hip}.s"; done
    work_base="$work/asm_base_renamed"
else
    work_base="$work/asm_base"
fi

bad=0
for f in $srcs; do
    s=${f%.hip}.s
    if cmp -s "$work_base/$s" "$work/asm_tree/$s"; then echo "identical  $f"
    elif [ ! -s "$work/asm_tree/$s" ] || [ ! -s "$work_base/$s" ]; then echo "NO ASSEMBLY $f (see $work/asm_*/$f.log)"; bad=$((bad + 1))
    else echo "DIFFERS    $f"; by_function "$s"; bad=$((bad + 1)); fi
done
echo "$bad of $(echo $srcs | wc -w) files differ from $base"
[ "$bad" -eq 0 ]
