"""cvtmi_flat_rerank and cvtmi_opq_search_refine at the C boundary and in the layers above it (CPU only: exports, header, argument
checks)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["cvtmi_flat_rerank", "cvtmi_flat_rerank_dev", "cvtmi_flat_last_rerank", "cvtmi_opq_search_refine", "cvtmi_opq_search_refine_dev"]
CVTMI_EINVAL = -1
K_MAX, RERANK_MAX = 2048, 4096


def test_symbols_are_exported():
    import cvt_amd
    lib = cvt_amd.lib()
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_header_declarations_compile_as_c99(tmp_path):
    src = tmp_path / "flat_rerank_decl.c"
    src.write_text('#include "cvtmi.h"\n'
                   "int main(void)\n{\n"
                   "    int (*a)(cvtmi_flat_t, const void *, int64_t, const int64_t *, int, int64_t, int, void *, int64_t *) = cvtmi_flat_rerank;\n"
                   "    int (*b)(cvtmi_flat_t, const void *, int64_t, const int64_t *, int, int64_t, int, void *, int64_t *, void *) = cvtmi_flat_rerank_dev;\n"
                   "    int (*c)(cvtmi_flat_t, int64_t *) = cvtmi_flat_last_rerank;\n"
                   "    int (*d)(cvtmi_opq_t, cvtmi_flat_t, const float *, int64_t, int, int, int, int, float *, int64_t *) = cvtmi_opq_search_refine;\n"
                   "    int (*e)(cvtmi_opq_t, cvtmi_flat_t, const float *, int64_t, int, int, int, int, float *, int64_t *, void *) = cvtmi_opq_search_refine_dev;\n"
                   "    return (a && b && c && d && e && CVTMI_RERANK_MAX == 4096) ? CVTMI_OK : CVTMI_EINVAL;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "cvtmi.h")).read()
    assert hdr.index("int cvtmi_flat_last_range_plan") < hdr.index("#define CVTMI_RERANK_MAX 4096") < hdr.index("int cvtmi_flat_rerank(")
    block = hdr[hdr.index("int cvtmi_flat_last_range_plan"):hdr.index("int cvtmi_opq_search_refine(")]
    for word in ("Candidates ", "Distance ", "Order ", "Labels ", "Limits ", "Concurrency", "bit for bit", "without signed overflow", "counts once",
                 '"rerank_rows_copy"', "SECOND copy", "EIGHT times", "0x7f800000", "CVTMI_EUNSUPPORTED", "RAW queries", "id_base"):
        assert word in block, word
    params = hdr[hdr.index("Per-handle parameters"):hdr.index("int cvtmi_flat_set_param")]
    assert '"rerank_rows_copy"' in params


def test_rerank_argument_checks_before_any_device_work():
    """Every CVTMI_EINVAL case of cvtmi_flat_rerank, on a NULL handle (nothing can have touched a device), through both entries; the
    output arrays keep their sentinels."""
    import cvt_amd
    lib = cvt_amd.lib()
    null = C.c_void_p(0)
    q = (C.c_float * 8)()
    cand = (C.c_int64 * 8)()
    d = (C.c_float * 4)(5.0, 5.0, 5.0, 5.0)
    i = (C.c_int64 * 4)(9, 9, 9, 9)
    cases = [
        (q, 2, cand, 4, 2, d, i),                     # NULL handle alone
        (null, 2, cand, 4, 2, d, i),                  # NULL q
        (q, 2, null, 4, 2, d, i),                     # NULL cand
        (q, 2, cand, 4, 2, null, i),                  # NULL dist
        (q, 2, cand, 4, 2, d, null),                  # NULL labels
        (q, -1, cand, 4, 2, d, i),                    # nq < 0
        (q, 2, cand, 4, 0, d, i),                     # k < 1
        (q, 2, cand, 4, K_MAX + 1, d, i),             # k > CVTMI_K_MAX
        (q, 2, cand, 0, 2, d, i),                     # R < 1
        (q, 2, cand, RERANK_MAX + 1, 2, d, i),        # R > CVTMI_RERANK_MAX
        (q, 0, cand, 4, 2, d, i),                     # a well-formed call of nothing: still no handle
    ]
    for base in (0, 10 ** 10, -2 ** 63):
        for qq, nq, cc, R, k, dd, ii in cases:
            args = (null, qq, C.c_int64(nq), cc, C.c_int(R), C.c_int64(base), C.c_int(k), dd, ii)
            assert lib.cvtmi_flat_rerank(*args) == CVTMI_EINVAL, (nq, R, k)
            assert lib.cvtmi_last_error()
            assert lib.cvtmi_flat_rerank_dev(*args, null) == CVTMI_EINVAL, (nq, R, k)
    assert list(d) == [5.0] * 4 and list(i) == [9] * 4
    out = (C.c_int64 * 4)(3, 3, 3, 3)
    assert lib.cvtmi_flat_last_rerank(null, out) == CVTMI_EINVAL and list(out) == [3] * 4
    assert lib.cvtmi_flat_set_param(null, b"rerank_rows_copy", C.c_int64(1)) == CVTMI_EINVAL


def test_refine_argument_checks_before_any_device_work():
    import cvt_amd
    lib = cvt_amd.lib()
    null = C.c_void_p(0)
    q = (C.c_float * 8)()
    d = (C.c_float * 4)(5.0, 5.0, 5.0, 5.0)
    i = (C.c_int64 * 4)(9, 9, 9, 9)
    cases = [
        (q, 2, 0, 2, 4, d, i),                # NULL handles alone
        (null, 2, 0, 2, 4, d, i),             # NULL q
        (q, 2, 0, 2, 4, null, i),             # NULL dist
        (q, 2, 0, 2, 4, d, null),             # NULL labels
        (q, -1, 0, 2, 4, d, i),               # nq < 0
        (q, 2, -1, 2, 4, d, i),               # nprobe < 0
        (q, 2, 3, 0, 4, d, i),                # k < 1
        (q, 2, 3, 5, 4, d, i),                # k > R
        (q, 2, 3, 2, K_MAX + 1, d, i),        # R > CVTMI_K_MAX
        (q, 0, 1, 2, 4, d, i),                # a well-formed call of nothing: still no handle
    ]
    for qq, nq, nprobe, k, R, dd, ii in cases:
        for rotate in (0, 1):
            args = (null, null, qq, C.c_int64(nq), C.c_int(rotate), C.c_int(nprobe), C.c_int(k), C.c_int(R), dd, ii)
            assert lib.cvtmi_opq_search_refine(*args) == CVTMI_EINVAL, (nq, nprobe, k, R)
            assert lib.cvtmi_last_error()
            assert lib.cvtmi_opq_search_refine_dev(*args, null) == CVTMI_EINVAL, (nq, nprobe, k, R)
    assert list(d) == [5.0] * 4 and list(i) == [9] * 4


def test_no_new_tuning_key():
    """the row-major copy is a per-handle parameter: the library-wide table does not know it"""
    import cvt_amd
    lib = cvt_amd.lib()
    for key in (b"rerank_rows_copy", b"flat_rerank_rows_copy"):
        assert lib.cvtmi_set_tuning(key, C.c_int64(1)) == CVTMI_EINVAL
    keys = [l for l in open(os.path.join(ROOT, "cvt_amd", "csrc", "tuning.def")).read().splitlines() if l.startswith("TUNE")]
    assert len(keys) == 68, len(keys)


def test_python_methods_exist():
    from cvt_amd import capi
    assert callable(getattr(capi.FlatIndex, "rerank"))
    assert callable(getattr(capi.FlatIndex, "last_rerank"))
    assert callable(getattr(capi.OpqIndex, "search_refine"))
