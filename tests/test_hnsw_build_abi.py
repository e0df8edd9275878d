"""CPU: the HNSW construction entries of the C ABI (include/cvtmi.h, "Graph construction on the GPU") are exported, declared in
plain C, reject bad arguments before any device work, and the hnsw_build tool names its GPU mode.  No GPU involved."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
SYMBOLS = ["cvtmi_hnsw_build", "cvtmi_hnsw_build_dev", "cvtmi_hnsw_save"]
EINVAL = -1


def test_library_exports_build_entries():
    import cvt_amd
    lib = cvt_amd.lib()
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_header_declarations_compile_as_c99(tmp_path):
    src = tmp_path / "hnsw_build_decl.c"
    src.write_text('#include "cvtmi.h"\n'
                   "int main(void)\n{\n"
                   "    int (*a)(const float *, int64_t, int, int, int, int, const uint64_t *, int, cvtmi_hnsw_t *) = cvtmi_hnsw_build;\n"
                   "    int (*b)(const float *, int64_t, int, int, int, int, const uint64_t *, int, cvtmi_hnsw_t *, void *) = "
                   "cvtmi_hnsw_build_dev;\n"
                   "    int (*c)(cvtmi_hnsw_t, void *, int64_t, int64_t *) = cvtmi_hnsw_save;\n"
                   "    return (a && b && c) ? CVTMI_OK : CVTMI_EINVAL;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)],
                   check=True)


def test_hnsw_build_usage_mentions_gpu():
    exe = os.path.join(BIN, "hnsw_build")
    assert os.path.exists(exe), "host CLIs not built: __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "usage: hnsw_build" in r.stdout and "gpu" in r.stdout and "gpu:<max_batch>" in r.stdout


X = np.zeros((8, 4), np.float32)


@pytest.mark.parametrize("n,D,metric,M,efc,max_batch,null_x,null_out", [
    (0, 4, 0, 8, 10, 0, False, False),     # n < 1
    (8, 0, 0, 8, 10, 0, False, False),     # D < 1
    (8, 4, 7, 8, 10, 0, False, False),     # unknown metric
    (8, 4, 2, 8, 10, 0, False, False),     # L2U8 is not a graph metric
    (8, 4, 1, 1, 10, 0, False, False),     # M < 2
    (8, 4, 1, 33, 40, 0, False, False),    # M > 32
    (8, 4, 0, 8, 0, 0, False, False),      # ef_construction < 1
    (8, 4, 0, 8, 10, -1, False, False),    # max_batch < 0
    (8, 4, 0, 8, 10, 0, True, False),      # NULL rows
    (8, 4, 0, 8, 10, 0, False, True),      # NULL out
])
def test_bad_arguments_are_einval(n, D, metric, M, efc, max_batch, null_x, null_out):
    import cvt_amd
    lib = cvt_amd.lib()
    x = C.c_void_p(0) if null_x else C.c_void_p(X.ctypes.data)
    for dev in (False, True):
        h = C.c_void_p(12345)
        out = None if null_out else C.byref(h)
        if dev:
            rc = lib.cvtmi_hnsw_build_dev(x, C.c_int64(n), C.c_int(D), C.c_int(metric), C.c_int(M), C.c_int(efc), C.c_void_p(0),
                                          C.c_int(max_batch), out, C.c_void_p(0))
        else:
            rc = lib.cvtmi_hnsw_build(x, C.c_int64(n), C.c_int(D), C.c_int(metric), C.c_int(M), C.c_int(efc), C.c_void_p(0),
                                      C.c_int(max_batch), out)
        assert rc == EINVAL
        if not null_out:
            assert h.value is None


def test_save_rejects_bad_handle():
    import cvt_amd
    lib = cvt_amd.lib()
    n = C.c_int64(-7)
    assert lib.cvtmi_hnsw_save(C.c_void_p(0), C.c_void_p(0), C.c_int64(0), C.byref(n)) == EINVAL
