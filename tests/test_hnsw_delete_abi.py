"""cvtmi_hnsw_mark_deleted and its companions at the C boundary and in the layers above it (CPU only: exports, header, argument checks,
method names, CLI usage).  No device is needed: a call that touched one here would answer CVTMI_EHIP, not CVTMI_EINVAL."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
SYMBOLS = ["cvtmi_hnsw_mark_deleted", "cvtmi_hnsw_mark_deleted_dev", "cvtmi_hnsw_unmark_deleted", "cvtmi_hnsw_unmark_deleted_dev",
           "cvtmi_hnsw_deleted_count", "cvtmi_hnsw_get_deleted", "cvtmi_hnsw_get_deleted_dev"]
CVTMI_EINVAL = -1


def test_symbols_are_exported():
    import cvt_amd
    lib = cvt_amd.lib()
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_header_declarations_compile_as_c99(tmp_path):
    src = tmp_path / "hnsw_delete_decl.c"
    src.write_text('#include "cvtmi.h"\n'
                   "int main(void)\n{\n"
                   "    int (*a)(cvtmi_hnsw_t, const int64_t *, int64_t, int64_t *) = cvtmi_hnsw_mark_deleted;\n"
                   "    int (*b)(cvtmi_hnsw_t, const int64_t *, int64_t, int64_t *, void *) = cvtmi_hnsw_mark_deleted_dev;\n"
                   "    int (*c)(cvtmi_hnsw_t, const int64_t *, int64_t, int64_t *) = cvtmi_hnsw_unmark_deleted;\n"
                   "    int (*d)(cvtmi_hnsw_t, const int64_t *, int64_t, int64_t *, void *) = cvtmi_hnsw_unmark_deleted_dev;\n"
                   "    int (*e)(cvtmi_hnsw_t, int64_t *) = cvtmi_hnsw_deleted_count;\n"
                   "    int (*f)(cvtmi_hnsw_t, uint64_t *, int64_t) = cvtmi_hnsw_get_deleted;\n"
                   "    int (*g)(cvtmi_hnsw_t, uint64_t *, int64_t, void *) = cvtmi_hnsw_get_deleted_dev;\n"
                   "    return (a && b && c && d && e && f && g) ? CVTMI_OK : CVTMI_EINVAL;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def _set_calls(lib, h, labels, n, changed):
    return [lambda: lib.cvtmi_hnsw_mark_deleted(h, labels, C.c_int64(n), changed),
            lambda: lib.cvtmi_hnsw_mark_deleted_dev(h, labels, C.c_int64(n), changed, C.c_void_p(0)),
            lambda: lib.cvtmi_hnsw_unmark_deleted(h, labels, C.c_int64(n), changed),
            lambda: lib.cvtmi_hnsw_unmark_deleted_dev(h, labels, C.c_int64(n), changed, C.c_void_p(0))]


def _get_calls(lib, h, mask, words):
    return [lambda: lib.cvtmi_hnsw_get_deleted(h, mask, C.c_int64(words)),
            lambda: lib.cvtmi_hnsw_get_deleted_dev(h, mask, C.c_int64(words), C.c_void_p(0))]


def test_null_handle_is_einval():
    import cvt_amd
    lib = cvt_amd.lib()
    null = C.c_void_p(0)
    lab = (C.c_int64 * 2)()
    mask = (C.c_uint64 * 2)()
    n = C.c_int64(0)
    calls = _set_calls(lib, null, lab, 2, C.byref(n)) + _set_calls(lib, null, null, 0, null) + _get_calls(lib, null, mask, 2) + [
        lambda: lib.cvtmi_hnsw_deleted_count(null, C.byref(n))]
    for i, call in enumerate(calls):
        lib.cvtmi_hnsw_save(null, null, C.c_int64(0), null)                # another message in between: the next one is the call's own
        assert b"null handle" not in lib.cvtmi_last_error()
        assert call() == CVTMI_EINVAL, i
        assert b"null handle" in lib.cvtmi_last_error(), (i, lib.cvtmi_last_error())


def test_wrong_arguments_are_refused_before_the_handle_is_used():
    """on memory that is no handle: a negative count, a NULL set with n_labels > 0, a NULL mask with mask_words > 0 and a NULL count
    pointer are named as such (the check comes before the handle's device is made current); good arguments reach the handle check"""
    import cvt_amd
    lib = cvt_amd.lib()
    bogus = C.create_string_buffer(4096)
    h = C.cast(bogus, C.c_void_p)
    null = C.c_void_p(0)
    lab = (C.c_int64 * 2)()
    mask = (C.c_uint64 * 2)()
    n = C.c_int64(0)
    for tag, (ll, cnt) in {"n_labels < 0": (lab, -1), "null labels": (null, 2)}.items():
        for i, call in enumerate(_set_calls(lib, h, ll, cnt, C.byref(n))):
            lib.cvtmi_hnsw_save(null, null, C.c_int64(0), null)
            assert call() == CVTMI_EINVAL, (tag, i)
            err = lib.cvtmi_last_error()
            assert b"bad arguments" in err and (b"cvtmi_hnsw_mark_deleted" in err or b"cvtmi_hnsw_unmark_deleted" in err), (tag, i, err)
    for tag, (mm, words) in {"mask_words < 0": (mask, -1), "null mask": (null, 2)}.items():
        for i, call in enumerate(_get_calls(lib, h, mm, words)):
            lib.cvtmi_hnsw_save(null, null, C.c_int64(0), null)
            assert call() == CVTMI_EINVAL, (tag, i)
            assert b"cvtmi_hnsw_get_deleted: bad arguments" in lib.cvtmi_last_error(), (tag, i, lib.cvtmi_last_error())
    lib.cvtmi_hnsw_save(null, null, C.c_int64(0), null)
    assert lib.cvtmi_hnsw_deleted_count(h, null) == CVTMI_EINVAL and b"null pointer" in lib.cvtmi_last_error()
    good = _set_calls(lib, h, lab, 2, C.byref(n)) + _set_calls(lib, h, lab, 2, null) + _set_calls(lib, h, null, 0, null) + \
        _get_calls(lib, h, mask, 2) + _get_calls(lib, h, null, 0) + [lambda: lib.cvtmi_hnsw_deleted_count(h, C.byref(n))]
    for i, call in enumerate(good):
        assert call() == CVTMI_EINVAL, i
        assert b"bad hnsw handle" in lib.cvtmi_last_error(), (i, lib.cvtmi_last_error())


def test_python_methods_exist():
    from cvt_amd import capi
    for name in ("mark_deleted", "unmark_deleted", "deleted_count", "deleted_mask"):
        assert callable(getattr(capi.HnswIndex, name)), name


def test_mirror_deletes():
    src = open(os.path.join(ROOT, "cvt_amd", "host", "hnswlib", "hnswalg.h")).read()
    for text in ("void markDelete(labeltype label)", "void unmarkDelete(labeltype label)", "size_t markDeleteBatch(", "size_t unmarkDeleteBatch(",
                 "cvtmi_hnsw_mark_deleted", "cvtmi_hnsw_unmark_deleted"):
        assert text in src, text


def test_hnsw_delete_usage(tmp_path):
    exe = os.path.join(BIN, "hnsw_delete")
    assert os.path.exists(exe), "host CLIs not built: __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "usage: hnsw_delete" in r.stdout and "--unmark" in r.stdout
    for extra in (["--mark"], ["--unmark", "more"], ["more", "--unmark"]):
        r = subprocess.run([exe, "in", "labels", "out"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage: hnsw_delete" in r.stderr, extra
    r = subprocess.run([exe, str(tmp_path / "missing.hnsw"), str(tmp_path / "missing.txt"), str(tmp_path / "out")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "cannot open" in r.stdout
