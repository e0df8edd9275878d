"""The IVF search at the C boundary and in the layers above it (CPU only: exports, header, argument checks, the host planner)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
SYMBOLS = ["cvtmi_opq_search_ivf", "cvtmi_opq_search_ivf_dev", "cvtmi_opq_ivf_plan", "cvtmi_opq_last_ivf_plan"]
CVTMI_EINVAL = -1


def test_symbols_are_exported():
    import cvt_amd
    lib = cvt_amd.lib()
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_header_declarations_compile_as_c99(tmp_path):
    src = tmp_path / "ivf_decl.c"
    src.write_text('#include "cvtmi.h"\n'
                   "int main(void)\n{\n"
                   "    int (*a)(cvtmi_opq_t, const float *, int64_t, int, int, int, float *, int64_t *) = cvtmi_opq_search_ivf;\n"
                   "    int (*b)(cvtmi_opq_t, const float *, int64_t, int, int, int, float *, int64_t *, void *) = cvtmi_opq_search_ivf_dev;\n"
                   "    int (*c)(int64_t, int, int, int64_t, int, int64_t *) = cvtmi_opq_ivf_plan;\n"
                   "    int (*d)(cvtmi_opq_t, int64_t *) = cvtmi_opq_last_ivf_plan;\n"
                   "    return (a && b && c && d) ? CVTMI_OK : CVTMI_EINVAL;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_einval_value_matches_header():
    import re
    hdr = open(os.path.join(ROOT, "include", "cvtmi.h")).read()
    m = re.search(r"CVTMI_EINVAL\s*=\s*(-?\d+)", hdr)
    assert m and int(m.group(1)) == CVTMI_EINVAL


def test_null_handle_is_einval():
    import cvt_amd
    lib = cvt_amd.lib()
    q = (C.c_float * 4)()
    d = (C.c_float * 4)()
    i = (C.c_int64 * 4)()
    assert lib.cvtmi_opq_search_ivf(C.c_void_p(0), q, C.c_int64(1), C.c_int(0), C.c_int(1), C.c_int(1), d, i) == CVTMI_EINVAL
    assert lib.cvtmi_opq_search_ivf_dev(C.c_void_p(0), q, C.c_int64(1), C.c_int(0), C.c_int(1), C.c_int(1), d, i, C.c_void_p(0)) == CVTMI_EINVAL
    assert b"null handle" in lib.cvtmi_last_error()
    assert lib.cvtmi_opq_last_ivf_plan(C.c_void_p(0), (C.c_int64 * 8)()) == CVTMI_EINVAL


def test_python_method_exists():
    from cvt_amd import capi
    assert callable(getattr(capi.OpqIndex, "search_ivf"))
    assert callable(getattr(capi.OpqIndex, "last_ivf_plan"))


def test_opq_search_usage_names_nprobe():
    exe = os.path.join(BIN, "opq_search")
    assert os.path.exists(exe), "host CLIs not built: __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "usage: opq_search" in r.stderr and "--nprobe" in r.stderr


def plan(nq, nprobe, k, longest, cus=256):
    import cvt_amd
    o = (C.c_int64 * 6)()
    assert cvt_amd.lib().cvtmi_opq_ivf_plan(C.c_int64(nq), C.c_int(nprobe), C.c_int(k), C.c_int64(longest), C.c_int(cus), o) == 0
    return dict(rule=o[0], G=o[1], groups=o[2], pieces=o[3], rpp=o[4], parts=o[5])


def test_planner_rules():
    """The grid rules the header documents: 256 CUs, two workgroups per CU wanted."""
    # a large batch: one workgroup per query, lists whole, no merge -- however long the longest list
    for longest in (0, 122, 40000):
        p = plan(5000, 16, 100, longest)
        assert (p["rule"], p["G"], p["groups"], p["pieces"], p["parts"]) == (1, 16, 1, 1, 1)
    # a handful of queries: one list per workgroup
    p = plan(7, 3, 10, 122)
    assert (p["rule"], p["G"], p["groups"], p["pieces"]) == (2, 1, 3, 1)
    # 64 queries x 16 lists: 8 groups of 2 give the 512 workgroups
    p = plan(64, 16, 10, 122)
    assert (p["rule"], p["G"], p["groups"], p["parts"]) == (2, 2, 8, 8)
    # one query, one long list: pieces of at least 1024 rows
    p = plan(1, 3, 100, 40000)
    assert p["rule"] == 3 and p["groups"] == 3 and p["rpp"] >= 1024 and p["rpp"] % 256 == 0
    assert p["pieces"] == -(-40000 // p["rpp"]) and p["pieces"] > 1
    # partial lists must fit 256 MB: 2 queries x 128 lists x 2048 is fine, 400 queries x 2 groups x 40 pieces x 2048 x 8 B is not
    p = plan(2, 128, 2048, 300)
    assert p["rule"] == 2 and p["groups"] == 128
    p = plan(100, 3, 2048, 4000000)
    assert 100 * p["parts"] * 2048 * 8 <= 256 << 20
    # every plan covers all probe slots and all rows
    for nq in (1, 2, 7, 64, 500, 1000, 5000):
        for nprobe in (1, 3, 16, 128):
            for longest in (0, 1, 255, 2567, 40000):
                p = plan(nq, nprobe, 100, longest)
                assert p["G"] * p["groups"] >= nprobe and p["G"] * (p["groups"] - 1) < nprobe
                assert p["pieces"] * p["rpp"] >= longest and p["pieces"] >= 1 and p["rpp"] >= 1
