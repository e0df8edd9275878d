"""cvtmi_hnsw_add and its companions at the C boundary and in the layers above it (CPU only: exports, header, argument checks, method
names, CLI usage).  No device is needed: a call that touched one here would answer CVTMI_EHIP, not CVTMI_EINVAL."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
SYMBOLS = ["cvtmi_hnsw_add", "cvtmi_hnsw_add_dev", "cvtmi_hnsw_reserve", "cvtmi_hnsw_level_draws", "cvtmi_hnsw_set_level_draws",
           "cvtmi_hnsw_last_add"]
CVTMI_EINVAL = -1


def test_symbols_are_exported():
    import cvt_amd
    lib = cvt_amd.lib()
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_header_declarations_compile_as_c99(tmp_path):
    src = tmp_path / "hnsw_add_decl.c"
    src.write_text('#include "cvtmi.h"\n'
                   "int main(void)\n{\n"
                   "    int (*a)(cvtmi_hnsw_t, const float *, int64_t, const uint64_t *, int) = cvtmi_hnsw_add;\n"
                   "    int (*b)(cvtmi_hnsw_t, const float *, int64_t, const uint64_t *, int, void *) = cvtmi_hnsw_add_dev;\n"
                   "    int (*c)(cvtmi_hnsw_t, int64_t) = cvtmi_hnsw_reserve;\n"
                   "    int (*d)(cvtmi_hnsw_t, int64_t *) = cvtmi_hnsw_level_draws;\n"
                   "    int (*e)(cvtmi_hnsw_t, int64_t) = cvtmi_hnsw_set_level_draws;\n"
                   "    int (*f)(cvtmi_hnsw_t, int64_t *) = cvtmi_hnsw_last_add;\n"
                   "    return (a && b && c && d && e && f) ? CVTMI_OK : CVTMI_EINVAL;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def _calls(lib, h, x, m, labels, max_batch):
    return [lambda: lib.cvtmi_hnsw_add(h, x, C.c_int64(m), labels, C.c_int(max_batch)),
            lambda: lib.cvtmi_hnsw_add_dev(h, x, C.c_int64(m), labels, C.c_int(max_batch), C.c_void_p(0))]


def test_null_handle_is_einval():
    import cvt_amd
    lib = cvt_amd.lib()
    null = C.c_void_p(0)
    x = (C.c_float * 8)()
    lab = (C.c_uint64 * 2)()
    out = (C.c_int64 * 4)()
    n = C.c_int64(0)
    calls = _calls(lib, null, x, 2, lab, 1) + _calls(lib, null, null, 0, null, 0) + [
        lambda: lib.cvtmi_hnsw_reserve(null, C.c_int64(10)),
        lambda: lib.cvtmi_hnsw_level_draws(null, C.byref(n)),
        lambda: lib.cvtmi_hnsw_set_level_draws(null, C.c_int64(3)),
        lambda: lib.cvtmi_hnsw_last_add(null, out),
    ]
    for i, call in enumerate(calls):
        lib.cvtmi_hnsw_save(null, null, C.c_int64(0), null)                # another message in between: the next one is the call's own
        assert b"null handle" not in lib.cvtmi_last_error()
        assert call() == CVTMI_EINVAL, i
        assert b"null handle" in lib.cvtmi_last_error(), (i, lib.cvtmi_last_error())


def test_wrong_arguments_are_refused_before_the_handle_is_used():
    """on memory that is no handle: m < 0, max_batch < 0 and NULL rows with m > 0 are named as such (the check comes before the
    handle's device is made current), good arguments reach the handle check; all CVTMI_EINVAL, each with its own text"""
    import cvt_amd
    lib = cvt_amd.lib()
    bogus = C.create_string_buffer(4096)
    h = C.cast(bogus, C.c_void_p)
    null = C.c_void_p(0)
    x = (C.c_float * 8)()
    lab = (C.c_uint64 * 2)()
    for tag, (xx, m, mb) in {"m < 0": (x, -1, 0), "max_batch < 0": (x, 2, -1), "null rows": (null, 2, 0)}.items():
        for i, call in enumerate(_calls(lib, h, xx, m, lab, mb)):
            lib.cvtmi_hnsw_save(null, null, C.c_int64(0), null)
            assert call() == CVTMI_EINVAL, (tag, i)
            assert b"cvtmi_hnsw_add: bad arguments" in lib.cvtmi_last_error(), (tag, i, lib.cvtmi_last_error())
    for i, call in enumerate(_calls(lib, h, x, 2, lab, 1) + _calls(lib, h, null, 0, null, 0)):
        assert call() == CVTMI_EINVAL, i
        assert b"bad hnsw handle" in lib.cvtmi_last_error(), (i, lib.cvtmi_last_error())
    n = C.c_int64(0)
    out = (C.c_int64 * 4)()
    for call, text in ((lambda: lib.cvtmi_hnsw_reserve(h, C.c_int64(-1)), b"negative"),
                       (lambda: lib.cvtmi_hnsw_reserve(h, C.c_int64(5)), b"bad hnsw handle"),
                       (lambda: lib.cvtmi_hnsw_set_level_draws(h, C.c_int64(-1)), b"negative"),
                       (lambda: lib.cvtmi_hnsw_set_level_draws(h, C.c_int64(5)), b"bad hnsw handle"),
                       (lambda: lib.cvtmi_hnsw_level_draws(h, null), b"null pointer"),
                       (lambda: lib.cvtmi_hnsw_level_draws(h, C.byref(n)), b"bad hnsw handle"),
                       (lambda: lib.cvtmi_hnsw_last_add(h, null), b"null pointer"),
                       (lambda: lib.cvtmi_hnsw_last_add(h, out), b"bad hnsw handle")):
        lib.cvtmi_hnsw_save(null, null, C.c_int64(0), null)
        assert call() == CVTMI_EINVAL, text
        assert text in lib.cvtmi_last_error(), (text, lib.cvtmi_last_error())


def test_python_methods_exist():
    from cvt_amd import capi
    for name in ("add", "reserve", "level_draws", "set_level_draws", "last_add"):
        assert callable(getattr(capi.HnswIndex, name)), name


def test_mirror_grows():
    src = open(os.path.join(ROOT, "cvt_amd", "host", "hnswlib", "hnswalg.h")).read()
    assert "void resizeIndex(size_t new_max_elements)" in src
    assert "cvtmi_hnsw_set_level_draws" in src and "cvtmi_hnsw_add" in src
    assert "the graph must be empty" not in src


def test_hnsw_add_usage():
    exe = os.path.join(BIN, "hnsw_add")
    assert os.path.exists(exe), "host CLIs not built: __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "usage: hnsw_add" in r.stdout and "gpu:<max_batch>" in r.stdout and "cont" in r.stdout
    # a bad space, mode or trailing word: usage errors before anything is opened
    for extra in (["cosine"], ["ip", "-", "fast"], ["ip", "-", "gpu1"], ["ip", "-", "gpu:-2"], ["ip", "-", "host", "continue"],
                  ["ip", "-", "host", "cont", "more"]):
        r = subprocess.run([exe, "in", "rows", "4", "out"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage: hnsw_add" in r.stderr, extra
