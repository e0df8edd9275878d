"""The piece arithmetic of the "scan_mfma" route (cvtmi_opq_mfma_plan, CPU only): every batch size has a plan -- the route must never turn
a valid search into an error -- its pieces cover the batch, and a piece's own scratch stays within the 1 GB the route allows itself."""
import ctypes as C

import pytest

import cvt_amd

GB = 1 << 30


def plan(D, n, nq, k, cap=4096, sample=2):
    lib = cvt_amd.lib()
    out = (C.c_int64 * 3)()
    rc = lib.cvtmi_opq_mfma_plan(C.c_int(D), C.c_int64(n), C.c_int64(nq), C.c_int(k), C.c_int(cap), C.c_int(sample), out)
    return rc, int(out[0]), int(out[1]), int(out[2])


@pytest.mark.parametrize("n", [20_000, 262_144, 1_000_000, 4_000_000, 8_000_000])
@pytest.mark.parametrize("k", [1, 100, 128])
def test_every_batch_has_a_plan(n, k):
    for D in (32, 128, 256):
        for sample in (1, 2, 3):
            for nq in (1, 33, 256, 257, 10_000, 200_000, 260_000, 320_000, 340_000, 400_000, 5_000_000, 2 ** 31 - 1):
                rc, per, pieces, total = plan(D, n, nq, k, sample=sample)
                assert rc == 0, (D, n, nq, k, sample)
                assert 1 <= per <= nq and pieces * per >= nq > (pieces - 1) * per, (D, n, nq, k, per, pieces)
                assert per == nq or per % 256 == 0, (nq, per)
                # what belongs to the call as a whole: flags, margins, the int8 queries, the rows' terms, the redo batch (a few MB)
                whole = nq * (D + 12) + n * 4 + (16 << 20)
                assert total - whole <= GB or per <= 256, (D, n, nq, k, sample, per, total)


def test_bad_arguments_are_refused():
    assert plan(48, 1000, 10, 10)[0] != 0
    assert plan(128, 1000, 10, 129)[0] != 0
    assert plan(128, 1000, 10, 10, cap=4097)[0] != 0
    assert plan(128, 0, 10, 10)[0] != 0
