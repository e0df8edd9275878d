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
