"""Host logic behind the uint8 stream's selection (flat_u8_stream_finish_kernel, cvt_amd/csrc/flat.hip): the slices per query against the
kernel's per-slice round tables (r_first[FIN_MAXR], r_off[FIN_MAXR + 1]).  Fewer slices mean more rounds per slice; the rule that
shrinks the slice count for 65 .. 128 queries used to be bounded for 64 slices only, and from about 41.7 M rows on a slice of the 8 it
chose spanned more rounds than the tables hold.  Pure host code: runs without a GPU (cvtmi_flat_describe_stream_finish)."""
import ctypes as C

import pytest

import cvt_amd

L2U8 = 2
WAVES = 1024          # wave minima per query (MSTREAM_BLOCKS * 4, flat_mfma.hip)
N_MAX = 2 ** 31 - 1


def plan(n, nq):
    lib = cvt_amd.lib()
    out = (C.c_int * 3)()
    assert lib.cvtmi_flat_describe_stream_finish(C.c_int64(n), C.c_int64(nq), out) == 0, (n, nq)
    return out[0], out[1], out[2]


def stream_applies(n, nq, D=128, k=10):
    lib = cvt_amd.lib()
    out = (C.c_int * 4)()
    cvt_amd.set_tuning("flat_u8_tfilter", 0)      # (the threshold filter would take some of these shapes first)
    try:
        assert lib.cvtmi_flat_describe_dispatch(L2U8, D, C.c_int64(n), C.c_int64(nq), k, out) == 0
    finally:
        cvt_amd.set_tuning("flat_u8_tfilter", 1)
    return bool(out[3])


def model_rounds(n, S):
    """the kernel's n_rounds, over every slice: chunk c = 32 rows, written by wave c % WAVES in its round c // WAVES"""
    c_total = (n + 31) // 32
    worst = 0
    for sl in range(S):
        c_lo, c_hi = c_total * sl // S, c_total * (sl + 1) // S
        if c_hi > c_lo:
            worst = max(worst, (c_hi - 1) // WAVES - c_lo // WAVES + 1)
    return worst


def rows_at(rounds, S):
    """about the row count from which a slice of S spans more than `rounds` rounds"""
    return rounds * WAVES * 32 * S


BREAKS = sorted({n + d for n in
                 [4096, 65_536, 1 << 20, 41_600_000, 41_800_000, 64 << 20, 100_000_000, 331_000_000, 333_447_168, 400_000_000, 1 << 30, N_MAX - 1] +
                 [rows_at(r, S) for r in (158, 159, 160) for S in (8, 16, 32, 64)]
                 for d in (-33, -1, 0, 1, 32, 33) if 4096 <= n + d <= N_MAX - 1} | {4096, N_MAX - 1})
QUERIES = sorted({1, 2, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 127, 128})


def test_rounds_per_slice_never_pass_the_tables():
    assert {41_600_000, 41_800_000, 64 << 20, (64 << 20) + 1} <= set(BREAKS)
    fin_maxr = plan(4096, 1)[2]
    assert fin_maxr == 160
    for n in BREAKS:
        for nq in QUERIES:
            S, rounds, maxr = plan(n, nq)
            assert S in (8, 16, 32, 64) and maxr == fin_maxr, (n, nq, S)
            assert rounds == model_rounds(n, S), (n, nq, S, rounds)       # the plan counts what the kernel counts
            if stream_applies(n, nq):
                assert rounds <= fin_maxr, (n, nq, S, rounds)
            else:                                                         # refused only where no slice count fits
                assert model_rounds(n, 64) > fin_maxr, (n, nq)
            # never halved past the bound -- and halved exactly as far as the measured rule asks wherever the bound allows it
            want = 64
            if n <= 64 << 20:
                while want > 8 and nq * want > 1024 and model_rounds(n, want // 2) <= fin_maxr:
                    want //= 2
            assert S == want, (n, nq, S, want)


@pytest.mark.parametrize("n", [41_600_000, 41_800_000, 64 << 20, (64 << 20) + 1])
@pytest.mark.parametrize("nq", [64, 65, 128])
def test_the_cells_the_old_rule_got_wrong(n, nq):
    """65 .. 128 queries over 41.7 M .. 64 Mi rows: the rule gave 8 slices of up to 257 rounds against tables of 160"""
    S, rounds, maxr = plan(n, nq)
    assert rounds <= maxr == 160 and stream_applies(n, nq)
    old = 64
    if n <= 64 << 20:
        while old > 4 and nq * old > 1024:
            old //= 2
    if model_rounds(n, old) <= maxr:
        assert S == old                     # where the old choice was sound it stands: 64 queries (16 slices), and 8 slices up to 41.6 M rows
    else:
        assert nq > 64 and 41_600_000 < n <= 64 << 20 and S == 16 and old == 8


def test_small_tables_keep_the_measured_slice_counts():
    for n in (4096, 262_176, 10_000_000):
        assert [plan(n, nq)[0] for nq in (1, 16, 17, 32, 33, 64, 65, 128)] == [64, 64, 32, 32, 16, 16, 8, 8]
    assert plan((64 << 20) + 1, 128)[0] == 64


def test_bad_arguments_are_refused():
    lib = cvt_amd.lib()
    out = (C.c_int * 3)()
    for n, nq in ((0, 1), (4096, 0), (4096, 129), (N_MAX, 1)):
        assert lib.cvtmi_flat_describe_stream_finish(C.c_int64(n), C.c_int64(nq), out) != 0
    assert lib.cvtmi_flat_describe_stream_finish(C.c_int64(4096), C.c_int64(1), None) != 0
