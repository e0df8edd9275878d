"""The range search at the C boundary and in the layers above it (CPU only: exports, header, status value, argument checks)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
SYMBOLS = ["cvtmi_opq_range_search_ivf", "cvtmi_opq_range_search_ivf_dev", "cvtmi_opq_last_range_plan"]
CVTMI_EINVAL, CVTMI_ESPACE = -1, -7


def test_symbols_are_exported():
    import cvt_amd
    lib = cvt_amd.lib()
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_header_declarations_compile_as_c99(tmp_path):
    src = tmp_path / "range_decl.c"
    src.write_text('#include "cvtmi.h"\n'
                   "int main(void)\n{\n"
                   "    int (*a)(cvtmi_opq_t, const float *, int64_t, int, int, float, int64_t, int64_t *, float *, int64_t *, int32_t *) = cvtmi_opq_range_search_ivf;\n"
                   "    int (*b)(cvtmi_opq_t, const float *, int64_t, int, int, float, int64_t, int64_t *, float *, int64_t *, int32_t *, void *) = cvtmi_opq_range_search_ivf_dev;\n"
                   "    int (*c)(cvtmi_opq_t, int64_t *) = cvtmi_opq_last_range_plan;\n"
                   "    return (a && b && c) ? CVTMI_OK : CVTMI_ESPACE;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_espace_value(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "cvtmi.h")).read()
    m = re.search(r"CVTMI_ESPACE\s*=\s*(-?\d+)", hdr)
    assert m and int(m.group(1)) == CVTMI_ESPACE
    src = tmp_path / "espace.c"                                            # ... and as the compiler sees it
    src.write_text('#include "cvtmi.h"\ntypedef char espace_is_minus_7[(CVTMI_ESPACE == -7) ? 1 : -1];\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)
    from cvt_amd import capi
    assert capi.ESPACE == CVTMI_ESPACE


def test_argument_checks_on_a_null_handle():
    """Every CVTMI_EINVAL case of the contract, on a NULL handle: nothing can have touched a device."""
    import cvt_amd
    lib = cvt_amd.lib()
    q = (C.c_float * 4)()
    lims = (C.c_int64 * 2)()
    d = (C.c_float * 4)()
    i = (C.c_int64 * 4)()
    v = (C.c_int32 * 4)()
    null = C.c_void_p(0)
    good = dict(h=null, q=q, nq=1, nprobe=1, radius=1.0, cap=4, lims=lims, d=d, i=i, v=v)
    cases = [{}, dict(q=null), dict(lims=null), dict(nq=-1), dict(nprobe=0), dict(cap=-1), dict(d=null), dict(i=null), dict(radius=float("nan")),
             dict(cap=0, d=null, i=null, v=null)]
    for change in cases:
        a = dict(good, **change)
        args = (a["h"], a["q"], C.c_int64(a["nq"]), C.c_int(0), C.c_int(a["nprobe"]), C.c_float(a["radius"]), C.c_int64(a["cap"]), a["lims"],
                a["d"], a["i"], a["v"])
        assert lib.cvtmi_opq_range_search_ivf(*args) == CVTMI_EINVAL, change
        assert lib.cvtmi_opq_range_search_ivf_dev(*args, C.c_void_p(0)) == CVTMI_EINVAL, change
        assert b"null handle" in lib.cvtmi_last_error()
    assert lib.cvtmi_opq_last_range_plan(null, (C.c_int64 * 8)()) == CVTMI_EINVAL


def test_tuning_key_is_registered():
    import cvt_amd
    cvt_amd.set_tuning("ivf_range_spill", 64)
    cvt_amd.set_tuning("ivf_range_spill", 1 << 30)
    cvt_amd.set_tuning("ivf_range_spill", 4096)
    assert cvt_amd.lib().cvtmi_set_tuning(b"ivf_range_spill", C.c_int64(-1)) == CVTMI_EINVAL


def test_python_methods_exist():
    from cvt_amd import capi
    assert callable(getattr(capi.OpqIndex, "range_search_ivf"))
    assert callable(getattr(capi.OpqIndex, "last_range_plan"))


def test_opq_search_usage_names_radius():
    exe = os.path.join(BIN, "opq_search")
    assert os.path.exists(exe), "host CLIs not built: __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--radius" in r.stderr
    # --radius without --nprobe is refused before anything is read
    r = subprocess.run([exe, "m", "d", "q", "r", "--radius", "0.5"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage: opq_search" in r.stderr
