"""cvtmi_opq_rank_videos at the C boundary and in the layers above it (CPU only: exports, header, argument checks)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
SYMBOLS = ["cvtmi_opq_rank_videos", "cvtmi_opq_rank_videos_dev", "cvtmi_opq_last_rank"]
CVTMI_EINVAL = -1


def test_symbols_are_exported():
    import cvt_amd
    lib = cvt_amd.lib()
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_header_declarations_compile_as_c99(tmp_path):
    src = tmp_path / "rank_decl.c"
    src.write_text('#include "cvtmi.h"\n'
                   "int main(void)\n{\n"
                   "    int (*a)(cvtmi_opq_t, const float *, const int64_t *, int64_t, int, int, int, int, float *, int64_t *, float *) = cvtmi_opq_rank_videos;\n"
                   "    int (*b)(cvtmi_opq_t, const float *, const int64_t *, int64_t, int, int, int, int, float *, int64_t *, float *, void *) = cvtmi_opq_rank_videos_dev;\n"
                   "    int (*c)(cvtmi_opq_t, int64_t *) = cvtmi_opq_last_rank;\n"
                   "    return (a && b && c) ? CVTMI_OK : CVTMI_EINVAL;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_argument_checks_on_a_null_handle():
    """A NULL handle is CVTMI_EINVAL from both entries whatever else is passed, and nothing is written."""
    import cvt_amd
    lib = cvt_amd.lib()
    q = (C.c_float * 64)()
    seg = (C.c_int64 * 3)(0, 1, 2)
    score = (C.c_float * 4)(7.0, 7.0, 7.0, 7.0)
    video = (C.c_int64 * 4)(7, 7, 7, 7)
    total = (C.c_float * 8)(*([7.0] * 8))
    last = (C.c_int64 * 4)(7, 7, 7, 7)
    null = C.c_void_p(0)
    for nseg in (0, 2, -1):
        args = (C.c_int64(nseg), C.c_int(1), C.c_int(3), C.c_int(4), C.c_int(2))
        assert lib.cvtmi_opq_rank_videos(null, q, seg, *args, score, video, total) == CVTMI_EINVAL
        assert b"null handle" in lib.cvtmi_last_error()
        assert lib.cvtmi_opq_rank_videos_dev(null, q, seg, *args, score, video, total, null) == CVTMI_EINVAL
        assert b"null handle" in lib.cvtmi_last_error()
    assert lib.cvtmi_opq_last_rank(null, last) == CVTMI_EINVAL
    assert list(score) == [7.0] * 4 and list(video) == [7] * 4 and list(total) == [7.0] * 8 and list(last) == [7] * 4


def test_tuning_table_is_unchanged():
    """the ranking's areas are bounded by the existing "ivf_part_cap_mb": no new tuning key"""
    keys = [l for l in open(os.path.join(ROOT, "cvt_amd", "csrc", "tuning.def")).read().splitlines() if l.startswith("TUNE")]
    assert len(keys) == 68, len(keys)


def test_header_describes_the_reuse_of_the_cap():
    hdr = open(os.path.join(ROOT, "include", "cvtmi.h")).read()
    at = hdr.index('"ivf_part_cap_mb" cvtmi_opq_search_ivf')                   # the key's entry in the table of tuning keys
    end = hdr.index('"scan_pad_m"', at)                                         # ... which ends where the next key begins
    assert "cvtmi_opq_rank_videos" in hdr[at:end]


def test_python_methods_exist():
    from cvt_amd import capi
    assert callable(getattr(capi.OpqIndex, "rank_videos"))
    assert callable(getattr(capi.OpqIndex, "last_rank"))


def test_opq_query_usage_names_batch():
    exe = os.path.join(BIN, "opq_query")
    assert os.path.exists(exe), "host CLIs not built: __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage: opq_query" in r.stderr and "[--batch]" in r.stderr
    r = subprocess.run([exe, "--batch", "m", "i"], capture_output=True, text=True, timeout=60)   # the flag is no positional argument
    assert r.returncode == 2 and "usage: opq_query" in r.stderr
