"""Removal from an OPQ index at the C boundary and in the layers above it (CPU only: exports, header, argument checks)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
SYMBOLS = ["cvtmi_opq_remove_videos", "cvtmi_opq_remove_videos_dev", "cvtmi_opq_remove_ids", "cvtmi_opq_remove_ids_dev"]
CVTMI_EINVAL = -1


def test_symbols_are_exported():
    import cvt_amd
    lib = cvt_amd.lib()
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_header_declarations_compile_as_c99(tmp_path):
    src = tmp_path / "remove_decl.c"
    src.write_text('#include "cvtmi.h"\n'
                   "int main(void)\n{\n"
                   "    int (*a)(cvtmi_opq_t, const int32_t *, int64_t, int, int64_t *, int64_t *) = cvtmi_opq_remove_videos;\n"
                   "    int (*b)(cvtmi_opq_t, const int32_t *, int64_t, int, int64_t *, int64_t *, void *) = cvtmi_opq_remove_videos_dev;\n"
                   "    int (*c)(cvtmi_opq_t, const int64_t *, int64_t, int64_t *, int64_t *) = cvtmi_opq_remove_ids;\n"
                   "    int (*d)(cvtmi_opq_t, const int64_t *, int64_t, int64_t *, int64_t *, void *) = cvtmi_opq_remove_ids_dev;\n"
                   "    return (a && b && c && d) ? CVTMI_OK : CVTMI_EINVAL;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_header_names_the_chunk_parameter():
    hdr = open(os.path.join(ROOT, "include", "cvtmi.h")).read()
    assert '"remove_chunk"' in hdr


def test_argument_checks_on_a_null_handle():
    """A NULL handle is CVTMI_EINVAL whatever else is passed: nothing can have touched a device."""
    import cvt_amd
    lib = cvt_amd.lib()
    v = (C.c_int32 * 4)()
    i = (C.c_int64 * 4)()
    removed = C.c_int64(7)
    null = C.c_void_p(0)
    for count in (0, 4, -1):
        assert lib.cvtmi_opq_remove_videos(null, v, C.c_int64(count), C.c_int(0), C.byref(removed), null) == CVTMI_EINVAL
        assert b"null handle" in lib.cvtmi_last_error()
        assert lib.cvtmi_opq_remove_videos_dev(null, v, C.c_int64(count), C.c_int(1), C.byref(removed), null, null) == CVTMI_EINVAL
        assert lib.cvtmi_opq_remove_ids(null, i, C.c_int64(count), C.byref(removed), null) == CVTMI_EINVAL
        assert lib.cvtmi_opq_remove_ids_dev(null, i, C.c_int64(count), C.byref(removed), null, null) == CVTMI_EINVAL
        assert b"null handle" in lib.cvtmi_last_error()
    assert removed.value == 7                                              # nothing was written
    assert lib.cvtmi_opq_set_param(null, b"remove_chunk", C.c_int64(1024)) == CVTMI_EINVAL


def test_tuning_table_is_unchanged():
    """the chunk size is a per-handle parameter: no new library-wide tuning key"""
    import cvt_amd
    assert cvt_amd.lib().cvtmi_set_tuning(b"remove_chunk", C.c_int64(1024)) == CVTMI_EINVAL
    keys = [l for l in open(os.path.join(ROOT, "cvt_amd", "csrc", "tuning.def")).read().splitlines() if l.startswith("TUNE")]
    assert len(keys) == 68, len(keys)


def test_python_methods_exist():
    from cvt_amd import capi
    assert callable(getattr(capi.OpqIndex, "remove_videos"))
    assert callable(getattr(capi.OpqIndex, "remove_ids"))


def test_opq_remove_usage():
    exe = os.path.join(BIN, "opq_remove")
    assert os.path.exists(exe), "host CLIs not built: __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage: opq_remove <model> <index_file> <out_dir> <video_id>..." in r.stderr
    r = subprocess.run([exe, "m", "i", "o", "three"], capture_output=True, text=True, timeout=60)   # refused before anything is read
    assert r.returncode == 2 and "bad video id" in r.stderr
