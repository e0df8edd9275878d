"""The inputs of test_gpu_opq_scan_tables.py are in the regime their names claim (CPU only).

Each case of scan_table_cases.py aims at one branch of the quantiser that builds the scans' 15-bit lower-bound tables
(range == 0, the 1e-37 clamp of the scale, a range that overflows fp32, a slack past 1024, denormal entries, row sums
at +inf over finite entries).  These predicates are conditions on the inputs -- the oracle's fp32 tables and row sums,
and the scale / bias / slack that follow from them (scan_table_cases.classify) -- so a later change of a seed or of
synth_model cannot quietly turn a case into an ordinary one."""
import numpy as np
import pytest

import scan_table_cases as sc

NATIVE_SHAPES = [(128, 8), (128, 4), (32, 8)]     # (D, M) of the native M = 8 / M = 4 scan's cases
NATIVE_CASES = ["constant", "x1e-18", "x1e19", "x1.5e19", "shift1e4"]


def _views(orc, name, D=128, M=16):
    """per query of the case: (tables, classification, the oracle's row sums as bit patterns, the row sums)"""
    books, q, codes = sc.make_case(name, D=D, M=M)
    out = []
    with np.errstate(all="ignore"):
        for f in range(q.shape[0]):
            lut = sc.lut_of(orc, books, q[f])
            sums = orc.adc_scan(lut, codes)
            out.append((lut, sc.classify(lut), sums.view(np.uint32), sums))
    return books, q, codes, out


def _distinct(bits):
    return len(np.unique(bits))


def test_model_tables_are_the_oracles(orc):
    """the numpy tables the offset search of `shift3000` uses are the oracle's, bit for bit"""
    for name in ("x1e-20", "shift1e4", "x1e19"):
        books, q, _ = sc.make_case(name)
        for f in (0, 8):
            assert np.array_equal(sc.lut_of(orc, books, q[f]).view(np.uint32), sc._tables(books, q[f]).view(np.uint32)), (name, f)


@pytest.mark.parametrize("name", sc.CASES)
def test_case_is_in_its_regime(orc, name):
    books, q, codes, views = _views(orc, name)
    n = codes.shape[0]
    assert q.shape == (sc.NQ, 128) and n == sc.ROWS and not np.isnan(q).any()
    if name in ("constant", "one_live"):
        live = None if name == "constant" else sc.ONE_LIVE_M
        for m in range(16):
            if m != live:
                assert np.array_equal(books[m], np.repeat(books[m, :1], 256, axis=0)), m
    if name == "x2.5e19":
        assert views[0][1]["nonfinite"] and sum(c["nonfinite"] for _, c, _, _ in views) >= 5
    for f, (lut, c, sbits, sums) in enumerate(views):
        tag = (name, f, float(c["range"]), float(c["scale"]), c["sl"], c["max_int_sum"], _distinct(sbits), int(np.isposinf(sums).sum()))
        print(tag)
        isum = c["qv"][np.arange(16)[None, :], codes].sum(axis=1)
        if name == "constant":
            assert c["range"] == 0 and c["scale"] == 1 and _distinct(sbits) == 1 and np.isfinite(sums).all(), tag
        elif name == "one_live":
            assert c["range"] > 0 and np.count_nonzero(c["mx"] - c["mn"]) == 1 and 100 < _distinct(sbits) < 300, tag
        elif name == "x1e-16":
            assert c["range"] > 0 and c["scale"] == c["pre_clamp"] and np.float32(1e-37) < c["scale"] < np.float32(1e-35), tag
            assert c["scale"] > sc.FLT_MIN, tag
        elif name in ("x1e-17", "x1e-18"):
            assert 0 < c["pre_clamp"] < np.float32(1e-37) and c["scale"] == np.float32(1e-37), tag
            assert 0 < c["max_int_sum"] < sc.MAXSUM // 4 and _distinct(sbits) > n - 64, tag
            assert c["lazy"] and c["sl"] == 35, tag
        elif name == "x1e-20":
            assert np.all(lut < sc.FLT_MIN) and np.any(lut > 0) and c["range"] > 0, tag
            assert c["max_int_sum"] == 0 and np.all(isum == 0) and _distinct(sbits) > 1000, tag
        elif name == "x1e-22":
            assert np.all(lut <= np.float32(16 * 1.4012985e-45)) and np.any(lut > 0) and c["range"] > 0, tag
            assert np.all(isum == 0) and 1 < _distinct(sbits) < 64, tag
        elif name == "x1e-23":
            assert np.all(lut == 0) and c["range"] == 0 and np.all(sums == 0), tag
        elif name == "x5e18":
            assert np.isfinite(lut).all() and np.isfinite(c["range"]) and c["range"] > np.float32(1e38) and np.isfinite(sums).all(), tag
            assert c["lazy"], tag
        elif name == "x1e19":
            assert np.isfinite(lut).all() and np.isposinf(c["range"]) and c["inv"] == 0, tag
            assert 1 <= np.isposinf(sums).sum() <= n - 128 and not np.isnan(sums).any(), tag
            assert np.all(isum == 0) and c["lazy"], tag
        elif name == "x1.5e19":
            assert np.isfinite(lut).all() and np.isposinf(c["range"]) and np.isposinf(sums).all(), tag
            assert c["lazy"] and c["sl"] == 35, tag
        elif name == "x2.5e19":
            assert np.isposinf(sums).all() and not np.isnan(lut).any(), tag
            assert c["nonfinite"] == bool(np.isposinf(lut).any()) and c["lazy"] == (not c["nonfinite"]), tag
        elif name == "shift3000":
            assert np.isfinite(lut).all() and 1000 <= c["sl"] < 1024 and c["lazy"], tag
            for k in (100, 128):   # the band [S_k, S_k + slack) of the lazy selection is hundreds of rows wide
                assert np.count_nonzero(isum < np.sort(isum)[k - 1] + c["sl"]) > k + 100, tag
        elif name == "shift1e4":
            assert np.isfinite(lut).all() and np.isfinite(sums).all() and c["sl"] >= 1024 and not c["lazy"], tag
            assert 16 < _distinct(sbits) < 200, tag
        elif name == "dominant":
            assert np.isfinite(lut).all() and c["lazy"] and 100 < _distinct(sbits) < 300, tag
            assert c["mx"][0] - c["mn"][0] > 1e5 * (c["mx"][1:] - c["mn"][1:]).max(), tag
        else:
            raise AssertionError(name)
        # what the kernels' proofs rest on, for every finite table: no carry out of a 16-bit sum
        assert 0 <= c["max_int_sum"] <= sc.MAXSUM, tag


def test_mixed_slots(orc):
    """nine regimes in one batch over plain books: the regime comes from the query alone"""
    books, q, codes, views = _views(orc, "mixed")
    n = codes.shape[0]
    assert q.shape[0] == 9
    plain = sc.make_case("constant")   # same seed: same base books before the case's own change
    assert books.shape == plain[0].shape

    def chk(f):
        lut, c, sbits, sums = views[f]
        tag = (f, float(c["range"]), float(c["scale"]), c["bias"], c["sl"], _distinct(sbits), int(np.isposinf(sums).sum()))
        print(tag)
        return lut, c, sbits, sums, tag

    for f in (0, 8):
        lut, c, sbits, sums, tag = chk(f)
        assert c["lazy"] and c["sl"] == 35 and c["bias"] > 0 and np.float32(1e-6) < c["scale"] < 1 and _distinct(sbits) > n - 64, tag
    assert np.array_equal(q[0], q[8])
    lut, c, sbits, sums, tag = chk(1)
    assert np.all(lut[:, sc.MIXED_CODEWORD] == 0) and c["bias"] == 0 and np.all(c["mn"] == 0) and c["lazy"], tag
    lut, c, sbits, sums, tag = chk(2)
    assert c["lazy"] and 100 <= c["sl"] < 1000, tag
    lut, c, sbits, sums, tag = chk(3)
    assert np.isfinite(lut).all() and c["sl"] >= 1024 and not c["lazy"] and c["range"] > 0 and _distinct(sbits) < 32, tag
    lut, c, sbits, sums, tag = chk(4)
    assert c["range"] == 0 and np.isfinite(sums).all() and np.all(lut > 1e30) and _distinct(sbits) == 1, tag
    lut, c, sbits, sums, tag = chk(5)
    assert np.isfinite(lut).all() and np.isposinf(sums).all(), tag
    lut, c, sbits, sums, tag = chk(6)
    assert np.isnan(q[6]).sum() == 1 and c["nonfinite"] and np.isnan(sums).all(), tag
    lut, c, sbits, sums, tag = chk(7)
    assert np.all(q[7].view(np.uint32) == 0x80000000) and c["lazy"] and c["sl"] == 35 and _distinct(sbits) > n - 64, tag
    assert list(sc.nan_free(q)) == [f != 6 for f in range(9)]


@pytest.mark.parametrize("D", sc.STEP_DIMS)
@pytest.mark.parametrize("name", sc.STEP_CASES)
def test_step_variants_keep_the_quantiser_branch(orc, name, D):
    """the same multipliers at sub-vector lengths 4 and 16 (the table kernels' generic path): the entries scale with the
    length, so the row-sum counts of the base shape do not carry over -- the branch of the quantiser does"""
    books, q, codes, views = _views(orc, name, D=D)
    assert books.shape == (16, 256, D // 16)
    for f, (lut, c, sbits, sums) in enumerate(views):
        tag = (name, D, f, float(c["range"]), float(c["scale"]), c["sl"], c["max_int_sum"])
        print(tag)
        assert np.isfinite(lut).all(), tag
        if name == "x1e-18":
            assert 0 < c["pre_clamp"] < np.float32(1e-37) and c["scale"] == np.float32(1e-37) and 0 < c["max_int_sum"] < 1000, tag
        elif name == "x1e19":
            assert np.isposinf(c["range"]) and c["inv"] == 0 and c["lazy"], tag
        else:
            assert c["sl"] >= 1024 and not c["lazy"] and np.isfinite(sums).all(), tag


@pytest.mark.parametrize("D,M", NATIVE_SHAPES)
def test_native_m_cases(orc, D, M):
    """M = 8 / M = 4 (adc_scan_p.hip): what each of the five cases still is at those shapes"""
    for name in NATIVE_CASES:
        books, q, codes, views = _views(orc, name, D=D, M=M)
        assert books.shape == (M, 256, D // M)
        for f, (lut, c, sbits, sums) in enumerate(views):
            tag = (name, D, M, f, float(c["range"]), float(c["scale"]), c["sl"], c["max_int_sum"], int(np.isposinf(sums).sum()))
            print(tag)
            assert np.isfinite(lut).all(), tag
            if name == "constant":
                assert c["range"] == 0 and _distinct(sbits) == 1, tag
            elif name == "x1e-18":
                assert 0 < c["pre_clamp"] < np.float32(1e-37) and 0 < c["max_int_sum"] < 1000, tag
            elif name == "x1e19":
                assert c["range"] > np.float32(1e38), tag          # finite or +inf: both sides of the overflow
            elif name == "x1.5e19":
                assert np.isposinf(c["range"]) and c["lazy"], tag
            else:
                assert c["sl"] >= 1024 and not c["lazy"], tag
