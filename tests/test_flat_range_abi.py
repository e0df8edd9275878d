"""Range search over a flat index at the C boundary and in the layers above it (CPU only: exports, header, argument checks)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
SYMBOLS = ["cvtmi_flat_range_search", "cvtmi_flat_range_search_dev", "cvtmi_flat_last_range_plan"]
CVTMI_EINVAL = -1


def test_symbols_are_exported():
    import cvt_amd
    lib = cvt_amd.lib()
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_header_declarations_compile_as_c99(tmp_path):
    src = tmp_path / "flat_range_decl.c"
    src.write_text('#include "cvtmi.h"\n'
                   "int main(void)\n{\n"
                   "    int (*a)(cvtmi_flat_t, const void *, int64_t, double, int64_t, int64_t *, void *, int64_t *) = cvtmi_flat_range_search;\n"
                   "    int (*b)(cvtmi_flat_t, const void *, int64_t, double, int64_t, int64_t *, void *, int64_t *, void *) = cvtmi_flat_range_search_dev;\n"
                   "    int (*c)(cvtmi_flat_t, int64_t *) = cvtmi_flat_last_range_plan;\n"
                   "    return (a && b && c) ? CVTMI_OK : CVTMI_ESPACE;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "cvtmi.h")).read()
    block = hdr[hdr.index("int cvtmi_flat_search_dev"):hdr.index("int cvtmi_flat_last_range_plan")]
    for word in ("Distance ", "Hit ", "Order ", "Labels ", "Outputs ", "Capacity ", "Concurrency", "no sharded form", "CVTMI_ESPACE", "bit for bit"):
        assert word in block, word
    params = hdr[hdr.index("Per-handle parameters"):hdr.index("int cvtmi_flat_set_param")]
    assert '"range_part_rows"' in params and '"range_spill"' in params


def _calls(lib):
    def host(h, q, nq, radius, cap, lims, d, i):
        return lib.cvtmi_flat_range_search(h, q, C.c_int64(nq), C.c_double(radius), C.c_int64(cap), lims, d, i)

    def dev(h, q, nq, radius, cap, lims, d, i):
        return lib.cvtmi_flat_range_search_dev(h, q, C.c_int64(nq), C.c_double(radius), C.c_int64(cap), lims, d, i, C.c_void_p(0))
    return host, dev


def test_argument_checks_before_any_device_work():
    """Every CVTMI_EINVAL case of the header, on a NULL handle (nothing can have touched a device), through both entries; the
    output arrays keep their sentinels."""
    import cvt_amd
    lib = cvt_amd.lib()
    null = C.c_void_p(0)
    q = (C.c_float * 8)()
    lims = (C.c_int64 * 3)(7, 7, 7)
    d = (C.c_float * 4)(5.0, 5.0, 5.0, 5.0)
    i = (C.c_int64 * 4)(9, 9, 9, 9)
    nan = float("nan")
    cases = [
        (null, q, 2, 1.0, 4, lims, d, i),       # NULL handle
        (null, null, 2, 1.0, 4, lims, d, i),    # NULL q
        (null, q, 2, 1.0, 4, null, d, i),       # NULL lims
        (null, q, -1, 1.0, 4, lims, d, i),      # nq < 0
        (null, q, 2, 1.0, -1, lims, d, i),      # cap < 0
        (null, q, 2, 1.0, 4, lims, null, i),    # NULL dist with cap > 0
        (null, q, 2, 1.0, 4, lims, d, null),    # NULL labels with cap > 0
        (null, q, 2, nan, 4, lims, d, i),       # NaN radius
        (null, q, 0, 1.0, 0, lims, null, null),  # a well-formed count-only call of nothing: still no handle
    ]
    for entry in _calls(lib):
        for args in cases:
            assert entry(*args) == CVTMI_EINVAL, args[2:5]
            assert lib.cvtmi_last_error()
    assert list(lims) == [7, 7, 7] and list(d) == [5.0] * 4 and list(i) == [9] * 4
    out = (C.c_int64 * 6)()
    assert lib.cvtmi_flat_last_range_plan(null, out) == CVTMI_EINVAL
    assert lib.cvtmi_flat_set_param(null, b"range_part_rows", C.c_int64(256)) == CVTMI_EINVAL
    assert lib.cvtmi_flat_set_param(null, b"range_spill", C.c_int64(0)) == CVTMI_EINVAL


def test_no_new_tuning_key():
    """part size and spill records are per-handle parameters: the library-wide table does not know them"""
    import cvt_amd
    lib = cvt_amd.lib()
    for key in (b"range_part_rows", b"range_spill", b"flat_range_spill"):
        assert lib.cvtmi_set_tuning(key, C.c_int64(1)) == CVTMI_EINVAL
    keys = [l for l in open(os.path.join(ROOT, "cvt_amd", "csrc", "tuning.def")).read().splitlines() if l.startswith("TUNE")]
    assert len(keys) == 68, len(keys)


def test_python_methods_exist():
    from cvt_amd import capi
    assert callable(getattr(capi.FlatIndex, "range_search"))
    assert callable(getattr(capi.FlatIndex, "last_range_plan"))


def test_bf_range_check_is_built():
    assert os.path.exists(os.path.join(BIN, "bf_range_check")), "host CLIs not built: __graft_entry__.build()"
