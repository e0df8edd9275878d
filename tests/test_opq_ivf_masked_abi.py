"""The masked IVF search at the C boundary and in the layers above it (CPU only: exports, header, argument checks, method names, CLI usage)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
SYMBOLS = ["cvtmi_opq_search_ivf_masked", "cvtmi_opq_search_ivf_masked_dev", "cvtmi_opq_mask_videos", "cvtmi_opq_mask_videos_dev",
           "cvtmi_opq_last_ivf_masked"]
CVTMI_EINVAL = -1


def test_symbols_are_exported():
    import cvt_amd
    lib = cvt_amd.lib()
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_header_declarations_compile_as_c99(tmp_path):
    src = tmp_path / "ivf_masked_decl.c"
    src.write_text('#include "cvtmi.h"\n'
                   "int main(void)\n{\n"
                   "    int (*a)(cvtmi_opq_t, const float *, int64_t, int, int, int, const uint64_t *, int64_t, float *, int64_t *) = cvtmi_opq_search_ivf_masked;\n"
                   "    int (*b)(cvtmi_opq_t, const float *, int64_t, int, int, int, const uint64_t *, int64_t, float *, int64_t *, void *) = cvtmi_opq_search_ivf_masked_dev;\n"
                   "    int (*c)(cvtmi_opq_t, const int32_t *, int64_t, uint64_t *, int64_t) = cvtmi_opq_mask_videos;\n"
                   "    int (*d)(cvtmi_opq_t, const int32_t *, int64_t, uint64_t *, int64_t, void *) = cvtmi_opq_mask_videos_dev;\n"
                   "    int (*e)(cvtmi_opq_t, int64_t *) = cvtmi_opq_last_ivf_masked;\n"
                   "    return (a && b && c && d && e) ? CVTMI_OK : CVTMI_EINVAL;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_null_handle_is_einval():
    import cvt_amd
    lib = cvt_amd.lib()
    q = (C.c_float * 4)()
    d = (C.c_float * 4)()
    i = (C.c_int64 * 4)()
    m = (C.c_uint64 * 4)()
    v = (C.c_int32 * 4)()
    null = C.c_void_p(0)
    calls = [
        lambda: lib.cvtmi_opq_search_ivf_masked(null, q, C.c_int64(1), C.c_int(0), C.c_int(1), C.c_int(1), m, C.c_int64(4), d, i),
        lambda: lib.cvtmi_opq_search_ivf_masked_dev(null, q, C.c_int64(1), C.c_int(0), C.c_int(1), C.c_int(1), m, C.c_int64(4), d, i, null),
        lambda: lib.cvtmi_opq_mask_videos(null, v, C.c_int64(4), m, C.c_int64(4)),
        lambda: lib.cvtmi_opq_mask_videos_dev(null, v, C.c_int64(4), m, C.c_int64(4), null),
        lambda: lib.cvtmi_opq_last_ivf_masked(null, (C.c_int64 * 8)()),
    ]
    for n, call in enumerate(calls):
        lib.cvtmi_opq_ntotal(null, null)                                   # another message in between: the next one is the call's own
        assert b"null handle" not in lib.cvtmi_last_error()
        assert call() == CVTMI_EINVAL, n
        assert b"null handle" in lib.cvtmi_last_error(), (n, lib.cvtmi_last_error())


def test_python_methods_exist():
    from cvt_amd import capi
    for name in ("search_ivf_masked", "mask_from_videos", "last_ivf_masked"):
        assert callable(getattr(capi.OpqIndex, name)), name


def test_opq_search_usage_names_videos():
    exe = os.path.join(BIN, "opq_search")
    assert os.path.exists(exe), "host CLIs not built: __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "usage: opq_search" in r.stderr and "--videos" in r.stderr
    # --videos needs --nprobe and excludes --radius: both are usage errors before anything is opened
    for extra in (["--videos", "v.txt"], ["--nprobe", "3", "--radius", "0.5", "--videos", "v.txt"]):
        r = subprocess.run([exe, "m", "d", "q", "r"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage: opq_search" in r.stderr, extra
