"""Every kernel launch goes through csrc/launch.h, and its grid rule holds (CPU only)."""
import ctypes as C
import glob
import os
import re

import pytest

import cvt_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cvt_amd", "csrc")

OK, EUNSUPPORTED = 0, -5


def test_status_codes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "cvtmi.h")).read()
    assert re.search(r"CVTMI_OK\s*=\s*0\b", hdr) and re.search(r"CVTMI_EUNSUPPORTED\s*=\s*-5\b", hdr)


def test_launch_h_is_the_only_file_that_launches():
    """no file of csrc other than launch.h launches a kernel itself (hipLaunchKernelGGL or triple chevrons) or asks the device for its
    CU count: a launch written out by hand has no grid check and shares its error check with its neighbours"""
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(files) > 40 and os.path.join(CSRC, "launch.h") in files
    bad = []
    for path in files:
        if os.path.basename(path) == "launch.h":
            continue
        text = open(path).read()
        for word in ("hipLaunchKernelGGL", "<<<", "multiProcessorCount"):
            if word in text:
                bad.append((os.path.basename(path), word))
    assert not bad, bad
    own = open(os.path.join(CSRC, "launch.h")).read()
    assert own.count("hipLaunchKernelGGL(") == 1 and "kernels.h" not in own and "std::function" not in own


def grid_status(x, y, z):
    lib = cvt_amd.lib()
    lib.cvtmi_describe_launch_grid.argtypes = [C.c_int64, C.c_int64, C.c_int64]
    lib.cvtmi_describe_launch_grid.restype = C.c_int
    rc = lib.cvtmi_describe_launch_grid(x, y, z)
    return rc, lib.cvtmi_last_error().decode(errors="replace")


@pytest.mark.parametrize("grid", [(1, 1, 1), (0x7fffffff, 1, 1), (1, 65535, 65535)])
def test_grids_within_the_limits_pass(grid):
    assert grid_status(*grid)[0] == OK


@pytest.mark.parametrize("grid", [(0x80000000, 1, 1), (1, 65536, 1), (1, 1, 65536), (0, 1, 1), (1, 0, 1), (-1, 1, 1), (1 << 40, 1, 1)])
def test_grids_outside_the_limits_are_refused_with_a_message(grid):
    """x above 0x7fffffff (the count that used to wrap in an (unsigned) cast), y or z above 65535, anything below 1"""
    rc, msg = grid_status(*grid)
    assert rc == EUNSUPPORTED
    bad = [v for v, hi in zip(grid, (0x7fffffff, 65535, 65535)) if v < 1 or v > hi][0]
    assert msg and str(bad) in msg, msg


# ---- the launch log (cvtmi_debug_launch_log_*, cvt_amd.launch_log): cvtmi_describe_launch_grid notes an accepted grid as launch() does ----

def raw_log():
    lib = cvt_amd.lib()
    for f in (lib.cvtmi_debug_launch_log_begin, lib.cvtmi_debug_launch_log_end, lib.cvtmi_debug_launch_log_read):
        f.restype = C.c_int64
    lib.cvtmi_debug_launch_log_read.argtypes = [C.c_int64, C.c_int64, C.c_void_p]
    return lib


def test_launch_log_is_empty_while_off_and_after_a_refused_grid():
    lib = raw_log()
    with cvt_amd.launch_log() as log:
        pass
    assert log == []
    assert grid_status(3, 1, 1)[0] == OK                       # log off: nothing is noted
    assert lib.cvtmi_debug_launch_log_read(0, 0, None) == 0
    with cvt_amd.launch_log() as log:
        assert grid_status(0x80000000, 1, 1)[0] == EUNSUPPORTED   # refused before the note, as a launch would be
        assert log == []                                       # (filled when the block ends)
        assert grid_status(5, 6, 7)[0] == OK
    assert log == [("cvtmi_describe_launch_grid", (5, 6, 7), 1, 0)]
    assert grid_status(9, 1, 1)[0] == OK                       # off again; the records stay readable until the next outermost begin
    assert lib.cvtmi_debug_launch_log_read(0, 0, None) == 1
    with cvt_amd.launch_log() as log:
        pass
    assert log == [] and lib.cvtmi_debug_launch_log_read(0, 0, None) == 0


def test_launch_log_blocks_nest():
    with cvt_amd.launch_log() as outer:
        grid_status(1, 1, 1)
        with cvt_amd.launch_log() as inner:
            grid_status(2, 1, 1)
            with cvt_amd.launch_log() as innermost:
                grid_status(3, 1, 1)
            grid_status(4, 1, 1)
        grid_status(5, 1, 1)                                   # the outer block is still on after the inner one ended
    assert [r[1][0] for r in innermost] == [3]
    assert [r[1][0] for r in inner] == [2, 3, 4]
    assert [r[1][0] for r in outer] == [1, 2, 3, 4, 5]
    lib = raw_log()
    assert lib.cvtmi_debug_launch_log_end() < 0 and "begin" in lib.cvtmi_last_error().decode()   # nothing open: refused


def test_launch_log_is_per_thread():
    """a thread's log sees its own launches only, and a begin on one thread leaves the others' logs off"""
    import threading
    a_on, main_done = threading.Event(), threading.Event()
    seen = {}

    def worker():
        with cvt_amd.launch_log() as log:
            grid_status(11, 1, 1)
            a_on.set()
            assert main_done.wait(30)
            grid_status(12, 1, 1)
        seen["worker"] = log

    t = threading.Thread(target=worker)
    t.start()
    assert a_on.wait(30)
    held = raw_log().cvtmi_debug_launch_log_read(0, 0, None)   # (what an earlier block of this thread left)
    assert grid_status(21, 1, 1)[0] == OK                      # main thread, its log off
    assert raw_log().cvtmi_debug_launch_log_read(0, 0, None) == held
    with cvt_amd.launch_log() as log:
        grid_status(22, 1, 1)
    main_done.set()
    t.join(30)
    assert [r[1][0] for r in seen["worker"]] == [11, 12] and [r[1][0] for r in log] == [22]


def test_launch_log_calls_touch_no_device():
    """begin / read / end are host bookkeeping: they succeed where there is no device (every device call fails there) and leave the
    thread's error text alone; read writes nothing past cap and reports the whole count"""
    lib = raw_log()
    assert grid_status(0, 1, 1)[0] == EUNSUPPORTED
    before = lib.cvtmi_last_error()
    assert lib.cvtmi_debug_launch_log_begin() == 0
    for x in (1, 2, 3):
        lib.cvtmi_describe_launch_grid(x, 1, 1)
    buf = (C.c_int64 * (3 * 13))(*([-7] * 39))                 # room for three 104-byte records
    assert lib.cvtmi_debug_launch_log_read(1, 1, buf) == 3     # one record from index 1
    assert buf[8] == 2 and buf[13] == -7                       # its grid x after the 64-byte name; the next record untouched
    assert lib.cvtmi_debug_launch_log_read(5, 3, buf) == 3 and buf[13] == -7   # past the end: nothing
    assert lib.cvtmi_debug_launch_log_end() == 3
    assert lib.cvtmi_last_error() == before and b"grid x = 0" in before   # no call above failed or reported anything
    assert lib.cvtmi_debug_launch_log_read(-1, 0, None) < 0 and b"launch_log_read" in lib.cvtmi_last_error()
    hdr = open(os.path.join(ROOT, "include", "cvtmi.h")).read()
    for name in ("cvtmi_debug_launch_log_begin", "cvtmi_debug_launch_log_end", "cvtmi_debug_launch_log_read", "cvtmi_launch_record"):
        assert name in hdr
    own = open(os.path.join(CSRC, "launch.h")).read()           # the off path: one pointer test, and the note comes before the launch
    assert own.index("log_launch(what, grid, block.x, lds);") < own.index("hipLaunchKernelGGL(")
