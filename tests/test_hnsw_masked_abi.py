"""The masked HNSW search at the C boundary and in the layers above it (CPU only: exports, header, argument checks, method names, CLI usage)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
SYMBOLS = ["cvtmi_hnsw_search_masked", "cvtmi_hnsw_search_masked_dev", "cvtmi_hnsw_search_adc_masked", "cvtmi_hnsw_search_adc_masked_dev",
           "cvtmi_hnsw_search_adc_rerank_masked", "cvtmi_hnsw_search_adc_rerank_masked_dev", "cvtmi_hnsw_mask_labels",
           "cvtmi_hnsw_mask_labels_dev", "cvtmi_hnsw_last_masked"]
CVTMI_EINVAL = -1


def test_symbols_are_exported():
    import cvt_amd
    lib = cvt_amd.lib()
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_header_declarations_compile_as_c99(tmp_path):
    src = tmp_path / "hnsw_masked_decl.c"
    src.write_text('#include "cvtmi.h"\n'
                   "int main(void)\n{\n"
                   "    int (*a)(cvtmi_hnsw_t, const float *, int64_t, int, int, const uint64_t *, int64_t, float *, int64_t *) = cvtmi_hnsw_search_masked;\n"
                   "    int (*b)(cvtmi_hnsw_t, const float *, int64_t, int, int, const uint64_t *, int64_t, float *, int64_t *, void *) = cvtmi_hnsw_search_masked_dev;\n"
                   "    int (*c)(cvtmi_hnsw_t, cvtmi_opq_t, const float *, int64_t, int, int, int, const uint64_t *, int64_t, float *, int64_t *) = cvtmi_hnsw_search_adc_masked;\n"
                   "    int (*d)(cvtmi_hnsw_t, cvtmi_opq_t, const float *, int64_t, int, int, int, const uint64_t *, int64_t, float *, int64_t *, void *) = cvtmi_hnsw_search_adc_masked_dev;\n"
                   "    int (*e)(cvtmi_hnsw_t, cvtmi_opq_t, const float *, int64_t, int, int, int, int, const uint64_t *, int64_t, float *, int64_t *) = cvtmi_hnsw_search_adc_rerank_masked;\n"
                   "    int (*f)(cvtmi_hnsw_t, cvtmi_opq_t, const float *, int64_t, int, int, int, int, const uint64_t *, int64_t, float *, int64_t *, void *) = cvtmi_hnsw_search_adc_rerank_masked_dev;\n"
                   "    int (*g)(cvtmi_hnsw_t, const int64_t *, int64_t, uint64_t *, int64_t) = cvtmi_hnsw_mask_labels;\n"
                   "    int (*h)(cvtmi_hnsw_t, const int64_t *, int64_t, uint64_t *, int64_t, void *) = cvtmi_hnsw_mask_labels_dev;\n"
                   "    int (*i)(cvtmi_hnsw_t, int64_t *) = cvtmi_hnsw_last_masked;\n"
                   "    return (a && b && c && d && e && f && g && h && i) ? CVTMI_OK : CVTMI_EINVAL;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_null_handle_is_einval():
    import cvt_amd
    lib = cvt_amd.lib()
    q = (C.c_float * 4)()
    d = (C.c_float * 4)()
    i = (C.c_int64 * 4)()
    m = (C.c_uint64 * 4)()
    null = C.c_void_p(0)
    one, ten, words = C.c_int64(1), C.c_int(10), C.c_int64(4)
    calls = [
        lambda: lib.cvtmi_hnsw_search_masked(null, q, one, C.c_int(1), ten, m, words, d, i),
        lambda: lib.cvtmi_hnsw_search_masked_dev(null, q, one, C.c_int(1), ten, m, words, d, i, null),
        lambda: lib.cvtmi_hnsw_search_adc_masked(null, null, q, one, C.c_int(1), C.c_int(1), ten, m, words, d, i),
        lambda: lib.cvtmi_hnsw_search_adc_masked_dev(null, null, q, one, C.c_int(1), C.c_int(1), ten, m, words, d, i, null),
        lambda: lib.cvtmi_hnsw_search_adc_rerank_masked(null, null, q, one, C.c_int(1), C.c_int(1), ten, ten, m, words, d, i),
        lambda: lib.cvtmi_hnsw_search_adc_rerank_masked_dev(null, null, q, one, C.c_int(1), C.c_int(1), ten, ten, m, words, d, i, null),
        lambda: lib.cvtmi_hnsw_mask_labels(null, i, C.c_int64(4), m, words),
        lambda: lib.cvtmi_hnsw_mask_labels_dev(null, i, C.c_int64(4), m, words, null),
        lambda: lib.cvtmi_hnsw_last_masked(null, (C.c_int64 * 4)()),
    ]
    for n, call in enumerate(calls):
        lib.cvtmi_hnsw_save(null, null, C.c_int64(0), null)                # another message in between: the next one is the call's own
        assert b"null handle" not in lib.cvtmi_last_error()
        assert call() == CVTMI_EINVAL, n
        assert b"null handle" in lib.cvtmi_last_error(), (n, lib.cvtmi_last_error())


def test_python_methods_exist():
    from cvt_amd import capi
    for name in ("search_masked", "search_adc_masked", "search_adc_rerank_masked", "mask_from_labels", "last_masked"):
        assert callable(getattr(capi.HnswIndex, name)), name


def test_mask_words_of_a_bool_array():
    """bit i & 63 of word i >> 6 = node i, little-endian; words pass through unchanged"""
    import numpy as np
    from cvt_amd import capi

    class Stub:
        ntotal = 70
    allowed = np.zeros(70, bool)
    allowed[[0, 63, 64, 69]] = True
    assert capi.HnswIndex._mask_words(Stub(), allowed, False).tolist() == [1 | 1 << 63, 1 | 1 << 5]
    same = np.array([5, 6, 7], dtype=np.uint64)
    assert capi.HnswIndex._mask_words(Stub(), same, False).tolist() == [5, 6, 7]


def test_mirror_has_the_filtered_overloads():
    src = open(os.path.join(ROOT, "cvt_amd", "host", "hnswlib", "hnswalg.h")).read()
    assert "searchKnn(void *query_data, size_t k, BaseFilterFunctor *isIdAllowed)" in src and "cvtmi_hnsw_search_masked" in src


def test_hnsw_search_usage_names_allow():
    exe = os.path.join(BIN, "hnsw_search")
    assert os.path.exists(exe), "host CLIs not built: __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "usage: hnsw_search" in r.stdout and "--allow" in r.stdout
    # --allow without its file, twice, or beside an unknown option: usage errors before anything is opened
    for extra in (["--allow"], ["ip", "--allow"], ["--allow", "a.txt", "--allow", "b.txt"], ["--deny", "a.txt"], ["ip", "l2"]):
        r = subprocess.run([exe, "i", "q", "4", "1", "1", "o"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage: hnsw_search" in r.stderr and "--allow" in r.stderr, extra
