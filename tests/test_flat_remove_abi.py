"""Removal from a flat index at the C boundary and in the layers above it (CPU only: exports, header, argument checks)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
SYMBOLS = ["cvtmi_flat_remove_labels", "cvtmi_flat_remove_labels_dev", "cvtmi_flat_set_param"]
CVTMI_EINVAL = -1


def test_symbols_are_exported():
    import cvt_amd
    lib = cvt_amd.lib()
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_header_declarations_compile_as_c99(tmp_path):
    src = tmp_path / "flat_remove_decl.c"
    src.write_text('#include "cvtmi.h"\n'
                   "int main(void)\n{\n"
                   "    int (*a)(cvtmi_flat_t, const int64_t *, int64_t, int64_t *, int64_t *) = cvtmi_flat_remove_labels;\n"
                   "    int (*b)(cvtmi_flat_t, const int64_t *, int64_t, int64_t *, int64_t *, void *) = cvtmi_flat_remove_labels_dev;\n"
                   "    int (*c)(cvtmi_flat_t, const char *, int64_t) = cvtmi_flat_set_param;\n"
                   "    return (a && b && c) ? CVTMI_OK : CVTMI_EINVAL;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "cvtmi.h")).read()
    block = hdr[hdr.index("int cvtmi_flat_reset"):hdr.index("int cvtmi_flat_set_param")]
    for word in ("Set ", "Result ", "Equivalence ", "Calling ", "Shards ", '"remove_chunk"', "numbers its rows by position"):
        assert word in block, word


def test_argument_checks_before_any_device_work():
    """A NULL handle is CVTMI_EINVAL whatever else is passed: nothing can have touched a device."""
    import cvt_amd
    lib = cvt_amd.lib()
    labels = (C.c_int64 * 4)()
    removed = C.c_int64(7)
    null = C.c_void_p(0)
    for count in (0, 4, -1):
        assert lib.cvtmi_flat_remove_labels(null, labels, C.c_int64(count), C.byref(removed), null) == CVTMI_EINVAL
        assert b"null handle" in lib.cvtmi_last_error()
        assert lib.cvtmi_flat_remove_labels_dev(null, labels, C.c_int64(count), C.byref(removed), null, null) == CVTMI_EINVAL
        assert b"null handle" in lib.cvtmi_last_error()
    assert removed.value == 7                                              # nothing was written
    assert lib.cvtmi_flat_set_param(null, b"remove_chunk", C.c_int64(1024)) == CVTMI_EINVAL


def test_tuning_table_is_unchanged():
    """the chunk size is a per-handle parameter: no new library-wide tuning key, and the version stays"""
    import cvt_amd
    lib = cvt_amd.lib()
    assert lib.cvtmi_set_tuning(b"remove_chunk", C.c_int64(1024)) == CVTMI_EINVAL
    keys = [l for l in open(os.path.join(ROOT, "cvt_amd", "csrc", "tuning.def")).read().splitlines() if l.startswith("TUNE")]
    assert len(keys) == 68, len(keys)
    assert lib.cvtmi_version() == 200


def test_python_methods_exist():
    from cvt_amd import capi
    assert callable(getattr(capi.FlatIndex, "remove_labels"))
    assert callable(getattr(capi.FlatIndex, "set_param"))


def test_bf_remove_check_is_built():
    assert os.path.exists(os.path.join(BIN, "bf_remove_check")), "host CLIs not built: __graft_entry__.build()"
    assert os.path.exists(os.path.join(BIN, "bf_sync_check"))
