"""cvtmi_flat_search_masked, cvtmi_flat_mask_labels and cvtmi_flat_last_masked at the C boundary and in the layers above it (CPU only:
exports, header, argument checks)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["cvtmi_flat_search_masked", "cvtmi_flat_search_masked_dev", "cvtmi_flat_mask_labels", "cvtmi_flat_mask_labels_dev", "cvtmi_flat_last_masked"]
CVTMI_EINVAL = -1
K_MAX = 2048


def test_symbols_are_exported():
    import cvt_amd
    lib = cvt_amd.lib()
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_header_declarations_compile_as_c99(tmp_path):
    src = tmp_path / "flat_masked_decl.c"
    src.write_text('#include "cvtmi.h"\n'
                   "int main(void)\n{\n"
                   "    int (*a)(cvtmi_flat_t, const void *, int64_t, int, const uint64_t *, int64_t, void *, int64_t *) = cvtmi_flat_search_masked;\n"
                   "    int (*b)(cvtmi_flat_t, const void *, int64_t, int, const uint64_t *, int64_t, void *, int64_t *, void *) = cvtmi_flat_search_masked_dev;\n"
                   "    int (*c)(cvtmi_flat_t, const int64_t *, int64_t, uint64_t *, int64_t) = cvtmi_flat_mask_labels;\n"
                   "    int (*d)(cvtmi_flat_t, const int64_t *, int64_t, uint64_t *, int64_t, void *) = cvtmi_flat_mask_labels_dev;\n"
                   "    int (*e)(cvtmi_flat_t, int64_t *) = cvtmi_flat_last_masked;\n"
                   "    return (a && b && c && d && e) ? CVTMI_OK : CVTMI_EINVAL;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "cvtmi.h")).read()
    assert hdr.index("int cvtmi_opq_search_refine_dev(") < hdr.index("int cvtmi_flat_search_masked(") < hdr.index("int cvtmi_flat_mask_labels(") \
        < hdr.index("int cvtmi_flat_last_masked(")
    # nothing went between the declarations the other ABI tests slice the header at
    between = hdr[hdr.index("int cvtmi_flat_search_dev"):hdr.index("int cvtmi_opq_search_refine(")]
    assert "masked" not in between
    block = hdr[hdr.index("int cvtmi_opq_search_refine_dev("):hdr.index("int cvtmi_flat_last_masked(")]
    for word in ("Mask ", "Distance ", "Order ", "Labels ", "Limits ", "Concurrency", "Shards", "In short", "bit for bit", "r & 63", "r >> 6", "ROW",
                 "insertion order", "cand_base = 0", "ceil(ntotal / 64)", "all-ones", "0x7f800000", "NaN", "id_base", "CVTMI_K_MAX", "INT32_MAX",
                 "2^32", "CVTMI_EINVAL", "nq == 0 does nothing", "all-zero mask", "shared lock", "never waits", "device pointers",
                 "cvtmi_topk_merge", "writes all mask_words", "cvtmi_flat_remove_labels", "n_labels == 0 clears", "Non-mutating",
                 "plain word operations", "no atomics", '"masked_parts"'):
        assert word in block, word
    tail = hdr[hdr.index("int cvtmi_flat_mask_labels_dev("):hdr.index("int cvtmi_flat_last_masked(")]
    for word in ("queries per workgroup", "parts per query group", "bytes of the row list", "kernel form", "queries in LDS", "queries in SGPRs",
                 "single bytes", "16-byte"):
        assert word in tail, word
    params = hdr[hdr.index("Per-handle parameters"):hdr.index("int cvtmi_flat_set_param")]
    assert '"masked_parts"' in params and "1 .. 1024" in params


def test_search_masked_argument_checks_before_any_device_work():
    """Every CVTMI_EINVAL case of cvtmi_flat_search_masked, on a NULL handle (nothing can have touched a device), through both entries;
    the output arrays keep their sentinels."""
    import cvt_amd
    lib = cvt_amd.lib()
    null = C.c_void_p(0)
    q = (C.c_float * 8)()
    mask = (C.c_uint64 * 2)(2 ** 64 - 1, 2 ** 64 - 1)
    d = (C.c_float * 4)(5.0, 5.0, 5.0, 5.0)
    i = (C.c_int64 * 4)(9, 9, 9, 9)
    cases = [
        (q, 2, 2, mask, 2, d, i),             # NULL handle alone
        (null, 2, 2, mask, 2, d, i),          # NULL q
        (q, 2, 2, null, 2, d, i),             # NULL mask
        (q, 2, 2, mask, 2, null, i),          # NULL dist
        (q, 2, 2, mask, 2, d, null),          # NULL labels
        (q, -1, 2, mask, 2, d, i),            # nq < 0
        (q, 2, 2, mask, -1, d, i),            # mask_words < 0
        (q, 2, 0, mask, 2, d, i),             # k < 1
        (q, 2, K_MAX + 1, mask, 2, d, i),     # k > CVTMI_K_MAX
        (q, 0, 2, mask, 2, d, i),             # a well-formed call of nothing: still no handle
    ]
    for qq, nq, k, mm, words, dd, ii in cases:
        args = (null, qq, C.c_int64(nq), C.c_int(k), mm, C.c_int64(words), dd, ii)
        assert lib.cvtmi_flat_search_masked(*args) == CVTMI_EINVAL, (nq, k, words)
        assert lib.cvtmi_last_error()
        assert lib.cvtmi_flat_search_masked_dev(*args, null) == CVTMI_EINVAL, (nq, k, words)
    assert list(d) == [5.0] * 4 and list(i) == [9] * 4
    out = (C.c_int64 * 4)(3, 3, 3, 3)
    assert lib.cvtmi_flat_last_masked(null, out) == CVTMI_EINVAL and list(out) == [3] * 4
    assert lib.cvtmi_flat_set_param(null, b"masked_parts", C.c_int64(2)) == CVTMI_EINVAL


def test_mask_labels_argument_checks_before_any_device_work():
    import cvt_amd
    lib = cvt_amd.lib()
    null = C.c_void_p(0)
    labels = (C.c_int64 * 4)(1, 2, 3, 4)
    mask = (C.c_uint64 * 2)(7, 7)
    cases = [
        (labels, 4, mask, 2),                 # NULL handle alone
        (null, 4, mask, 2),                   # NULL set with a positive count
        (labels, -1, mask, 2),                # a negative count
        (labels, 4, null, 2),                 # NULL mask with words to write
        (labels, 4, mask, -1),                # mask_words < 0
        (null, 0, mask, 2),                   # a well-formed empty set: still no handle
    ]
    for ll, n, mm, words in cases:
        args = (null, ll, C.c_int64(n), mm, C.c_int64(words))
        assert lib.cvtmi_flat_mask_labels(*args) == CVTMI_EINVAL, (n, words)
        assert lib.cvtmi_last_error()
        assert lib.cvtmi_flat_mask_labels_dev(*args, null) == CVTMI_EINVAL, (n, words)
    assert list(mask) == [7, 7]


def test_no_new_tuning_key():
    """the parts are a per-handle parameter: the library-wide table does not know them"""
    import cvt_amd
    lib = cvt_amd.lib()
    for key in (b"masked_parts", b"flat_masked_parts"):
        assert lib.cvtmi_set_tuning(key, C.c_int64(1)) == CVTMI_EINVAL
    keys = [l for l in open(os.path.join(ROOT, "cvt_amd", "csrc", "tuning.def")).read().splitlines() if l.startswith("TUNE")]
    assert len(keys) == 68, len(keys)


def test_python_methods_exist():
    from cvt_amd import capi
    assert callable(getattr(capi.FlatIndex, "search_masked"))
    assert callable(getattr(capi.FlatIndex, "mask_from_labels"))
    assert callable(getattr(capi.FlatIndex, "last_masked"))


def test_bool_masks_pack_little_endian():
    """bit r & 63 of word r >> 6 is row r (the packing needs no handle beyond ntotal)"""
    import numpy as np
    from cvt_amd import capi

    class Stub:
        ntotal = 130
    m = np.zeros(130, dtype=bool)
    m[[0, 63, 64, 129]] = True
    words = capi.FlatIndex._mask_words(Stub(), m, False)
    assert words.dtype == np.uint64 and words.tolist() == [1 | (1 << 63), 1, 2]
    same = np.array([5, 6, 7], dtype=np.uint64)
    assert capi.FlatIndex._mask_words(Stub(), same, False).tolist() == [5, 6, 7]


def test_mirror_and_self_check_are_built():
    src = open(os.path.join(ROOT, "cvt_amd", "host", "hnswlib", "bruteforce.h")).read()
    assert "struct BaseFilterFunctor" in src and "BaseFilterFunctor *isIdAllowed" in src and "cvtmi_flat_search_masked" in src
    mk = open(os.path.join(ROOT, "cvt_amd", "host", "Makefile")).read()
    clis = [l for l in mk.splitlines() if l.startswith("CLIS")][0]
    assert "bf_masked_check" in clis.split()
    exe = os.path.join(ROOT, "cvt_amd", "bin", "bf_masked_check")
    assert os.path.isfile(exe) and os.access(exe, os.X_OK)
