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


# The plans the cases of tests/test_gpu_opq_mfma_pieces.py are about, (D, rows, queries, k, list cap) -> (queries per piece, pieces): a change
# of the sizing that moves one of them takes that GPU case's premise away -- choose its batch anew there, then correct the figures here.
# How the pieces are laid out (chunks x queries per chunk; spx 8 from three chunks on, 16 at two, 32 at one):
#   8229 x 513: 3 x 192   600: 3 x 224   1100: 5 x 224   1536: 3 x 256 twice   1537: 4 x 256, then 513 = 3 x 192   1700: 4 x 256, then 676 = 3 x 256
#   2100: 5 x 256, then 820 = 4 x 224   2500: 3 x 256 three times, then 196 = 1 x 224   3100: 4 x 256 three times, then 28 = 1 x 32
#   20000 x 3100: 7 x 256, then 1308 = 6 x 224   97 x 300: 1 x 256, then 44 = 1 x 64   262149 x 4096: 16 x 256
GPU_CASE_PLANS = [
    ((128, 8229, 513, 100, 4096), (513, 1)), ((128, 8229, 600, 100, 4096), (600, 1)), ((128, 8229, 600, 10, 4096), (600, 1)),
    ((128, 8229, 1100, 100, 4096), (1100, 1)),
    ((128, 8229, 1536, 100, 4096), (768, 2)), ((128, 8229, 1537, 100, 4096), (1024, 2)), ((128, 8229, 1700, 100, 4096), (1024, 2)),
    ((128, 8229, 1700, 128, 4096), (1024, 2)), ((128, 8229, 2100, 10, 4096), (1280, 2)), ((128, 8229, 2100, 1, 4096), (1280, 2)),
    ((128, 8229, 2500, 128, 4096), (768, 4)), ((128, 8229, 3100, 100, 4096), (1024, 4)), ((128, 20000, 3100, 100, 4096), (1792, 2)),
    ((128, 97, 300, 1, 4096), (256, 2)),
    ((128, 8229, 1700, 100, 2), (1024, 2)), ((128, 8229, 3100, 10, 2), (1792, 2)), ((128, 97, 300, 100, 2), (256, 2)),
    ((32, 8229, 40, 50, 4096), (40, 1)), ((32, 8229, 600, 50, 4096), (600, 1)), ((96, 8229, 40, 50, 4096), (40, 1)),
    ((96, 8229, 600, 50, 4096), (600, 1)), ((96, 8229, 1700, 50, 4096), (1024, 2)), ((256, 8229, 40, 50, 4096), (40, 1)),
    ((256, 8229, 600, 50, 4096), (600, 1)),
    ((128, 262149, 4096, 100, 4096), (4096, 1)),
    ((128, 1_000_000, 10_000, 100, 4096), (5120, 2)),   # the headline: 5120 + 4880 queries
]


@pytest.mark.parametrize("case,want", GPU_CASE_PLANS)
def test_plans_the_gpu_cases_rely_on(case, want):
    D, n, nq, k, cap = case
    rc, per, pieces, _ = plan(D, n, nq, k, cap=cap)
    assert rc == 0 and (per, pieces) == want, (case, per, pieces)


def test_bad_arguments_are_refused():
    assert plan(48, 1000, 10, 10)[0] != 0
    assert plan(128, 1000, 10, 129)[0] != 0
    assert plan(128, 1000, 10, 10, cap=4097)[0] != 0
    assert plan(128, 0, 10, 10)[0] != 0
