"""The ADC scan kernels at the edges of their 15-bit lower-bound tables, against the oracle, bit for bit.

Every fast scan is a filter over integer lower bounds of the fp32 distance tables; each query's tables are quantised
with their own scale / bias / slack (adc_scan16.h scan16_query_params / scan16_quantise: one rule, called by
scan16q_build_tables<NT, M> for adc_scan16q / 16a / 16p and by adc_scan_h.hip scan16h_prep_kernel; each form still builds
and reads its tables its own way, so each is run here) and every later stage trusts those numbers: the filter threshold, the lazy
selection, the seed and 16h histograms, the packed sums.  The cases of scan_table_cases.py (pinned to their regimes by
test_scan_table_regimes.py) reach the branches ordinary data never does: range == 0, the 1e-37 clamp, a range that
overflows fp32 (inv_scale 0, scale_eff +inf), a slack past 1024 on finite tables, denormal entries, row sums at +inf
over finite entries.  There every integer sum may be 0 (spill areas fill, histograms hold one bin), bands are as wide
as the table and exact keys are all +inf.

Reference: orc.adc_search -- fp32 sum over m ascending, the k smallest (score, id); +inf rows are real rows and come
back with their ids in id order before any (+inf, -1) padding.  No tolerance: ids with np.array_equal, distances by
bit pattern.  A query with a NaN component only has to leave the others of its batch alone."""
import numpy as np
import pytest

import scan_table_cases as sc
from conftest import bits

pytestmark = pytest.mark.gpu

KS = (1, 100, 128)
ALL_CASES = sc.CASES + ["mixed"]
NATIVE_SHAPES = [(128, 8), (128, 4), (32, 8)]     # (D, M): steps 16 / 32 at D = 128, step 4 at M = 8
NATIVE_CASES = ["constant", "x1e-18", "x1e19", "x1.5e19", "shift1e4"]
SMALL_CASES = ["mixed", "constant", "x1e-20", "x1.5e19"]
BIGK_CASES = ["mixed", "one_live", "x1e19", "shift1e4"]


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()  # raises if the HIP library is missing: there is no fallback
    return cvt_amd


class Case:
    """one case's inputs, its index on the device and its oracle answers (computed once per k, shared, never written)"""

    def __init__(self, amd, orc, name, D=128, M=16, rows=sc.ROWS, **kw):
        self.key = (name, D, M, rows)
        self.orc = orc
        self.books, self.q, self.codes = sc.make_case(name, D=D, M=M, rows=rows)
        self.ok = sc.nan_free(self.q)
        self.idx = amd.OpqIndex(np.zeros((1, D), np.float32), self.books, **kw)
        self.idx.add_codes(self.codes)
        self.idx.set_param("profile", 1)

    def expect(self, k, nq=None, q_rot=None, tag=""):
        q = self.q if q_rot is None else q_rot
        q = q if nq is None else q[:nq]
        return sc.oracle_search(self.orc, self.key + (tag,), self.books, q, self.codes, k)

    def check(self, k, what, q=None, nq=None, q_rot=None, tag="", rotate=False):
        qs = self.q if q is None else q
        qs = qs if nq is None else qs[:nq]
        od, oi = self.expect(k, nq, q_rot, tag)
        d, i = self.idx.search(np.ascontiguousarray(qs), k, rotate=rotate)
        ok = self.ok[:qs.shape[0]]
        bad = [f for f in np.flatnonzero(ok) if not (np.array_equal(i[f], oi[f]) and np.array_equal(bits(d[f]), bits(od[f])))]
        assert not bad, (self.key, what, "k", k, "queries", bad, "first", _first_diff(d[bad[0]], i[bad[0]], od[bad[0]], oi[bad[0]]))

    def close(self):
        self.idx.close()


def _first_diff(d, i, od, oi):
    p = int(np.flatnonzero((i != oi) | (bits(d) != bits(od)))[0])
    return dict(pos=p, got=(float(d[p]), int(i[p])), want=(float(od[p]), int(oi[p])))


def _scan_shape(c, qtile=8, splits=None):
    """the launch the last search took: a dispatch change must not send a case to the fp32 kernels unnoticed"""
    ls = c.idx.last_scan()
    assert ls["qtile"] == qtile, (c.key, ls)
    if splits:
        assert ls["splits"] == splits, (c.key, ls)


@pytest.mark.parametrize("name", ALL_CASES)
def test_control_fp32_kernel(amd, orc, name):
    """scan_variant 0, the fp32 row-per-lane kernel: nothing is quantised -- the oracle and the index agree on the case itself"""
    c = Case(amd, orc, name)
    try:
        c.idx.set_param("scan_variant", 0)
        for k in KS:
            c.check(k, "variant 0")
    finally:
        c.close()


@pytest.mark.parametrize("variant", [3, 4, 5])
@pytest.mark.parametrize("name", ALL_CASES)
def test_scan16q_16a(amd, orc, name, variant):
    """adc_scan16q (3: 1024 threads, 4: 512) and adc_scan16a (5): whole groups and three row splits that share their thresholds,
    lazy selection on and off; variant 3 in three splits once more without the seed histogram"""
    c = Case(amd, orc, name)
    try:
        c.idx.set_param("scan_variant", variant)
        for splits in (1, 3):
            for lazy in (1, 0):
                c.idx.set_param("splits", splits); c.idx.set_param("scan_lazy", lazy)
                for k in KS:
                    c.check(k, ("variant", variant, "splits", splits, "lazy", lazy))
                    _scan_shape(c, 8, splits)
        if variant == 3:
            c.idx.set_param("splits", 3); c.idx.set_param("scan_lazy", 1)
            with sc.tuning(amd, scan_seed=0):
                for k in KS:
                    c.check(k, ("variant 3, splits 3, no seed",))
                    _scan_shape(c, 8, 3)
    finally:
        c.close()


@pytest.mark.parametrize("name", ALL_CASES)
def test_scan16h(amd, orc, name):
    """adc_scan16h (scan_variant 6): tables from scan16h_prep_kernel, spill areas, shared histograms; the planner's own item table
    and three forced row splits"""
    c = Case(amd, orc, name)
    try:
        c.idx.set_param("scan_variant", 6)
        for splits in (0, 3):
            c.idx.set_param("splits", splits)
            for k in KS:
                c.check(k, ("variant 6", "splits", splits))
                _scan_shape(c, 8, splits)
    finally:
        c.close()


@pytest.mark.parametrize("D", sc.STEP_DIMS)
@pytest.mark.parametrize("name", sc.STEP_CASES)
def test_other_sub_vector_lengths(amd, orc, name, D):
    """sub-vector lengths 4 and 16: the generic path of the table kernels (lut_kernel for adc_scan16q, scan16h_prep_kernel's own loop)"""
    c = Case(amd, orc, name, D=D)
    try:
        for variant, splits in ((3, 1), (3, 3), (6, 0), (6, 3), (0, 0)):
            c.idx.set_param("scan_variant", variant); c.idx.set_param("splits", splits)
            for k in KS:
                c.check(k, ("D", D, "variant", variant, "splits", splits))
                if variant:
                    _scan_shape(c, 8, splits)
    finally:
        c.close()


@pytest.mark.parametrize("form", ["packed", "padded"])
@pytest.mark.parametrize("D,M", NATIVE_SHAPES)
@pytest.mark.parametrize("name", NATIVE_CASES)
def test_native_m8_m4(amd, orc, name, D, M, form):
    """M = 8 / M = 4: the native packed scan (adc_scan_p.hip, scan16q_build_tables<NT, M>) and the rows padded to 16 bytes with all-zero
    tables behind the model's own (adc_scan16q: the range comes from the real tables only)"""
    c = Case(amd, orc, name, D=D, M=M)
    try:
        with sc.tuning(amd, scan_packed_m=1 if form == "packed" else 0, scan_pad_m=1):
            for splits in (0, 3):
                c.idx.set_param("splits", splits)
                for k in KS:
                    c.check(k, (form, "D", D, "M", M, "splits", splits))
                    _scan_shape(c, 8, splits)
    finally:
        c.close()


@pytest.mark.parametrize("nq", [1, 8, 9])
@pytest.mark.parametrize("name", SMALL_CASES)
def test_small_batch_path(amd, orc, name, nq):
    """launch_adc_scan_small (1 .. 128 queries on >= 65 536 rows, default dispatch): global bound from a histogram pass, candidate
    lists, selection by the last workgroup.  The path cannot be observed from outside: switched on and switched off must each
    give the oracle's lists."""
    c = Case(amd, orc, name, rows=sc.ROWS_BIG)
    try:
        for small in (1, 0):
            c.idx.set_param("scan_small", small)
            for k in KS:
                c.check(k, ("scan_small", small, "nq", nq), nq=nq, tag="nq%d" % nq)
    finally:
        c.close()


@pytest.mark.parametrize("nq", [1, 8, 9])
def test_small_batch_path_fused_rotation(amd, orc, nq):
    """`mixed` behind a dense rotation: the small-batch path rotates inside its table kernel (the k-ordered fmaf chain), the
    ordinary path through the rotation kernel -- the same tables either way"""
    from cvt_amd import synth
    R = synth.random_rotation(128, seed=5)
    c = Case(amd, orc, "mixed", rows=sc.ROWS_BIG, R=R)
    try:
        with np.errstate(all="ignore"):
            raw = (c.q.astype(np.float64) @ R.astype(np.float64)).astype(np.float32)     # y = R x brings them back (up to rounding)
        raw[6] = c.q[6]                                                                   # still ONE NaN component
        raw[7] = c.q[7]                                                                   # still every component -0.0
        raw[8] = raw[0]
        q_rot = orc.rotate_fma(R, raw)
        c.ok = sc.nan_free(q_rot)
        assert list(c.ok) == [f != 6 for f in range(9)]
        for small in (1, 0):
            c.idx.set_param("scan_small", small)
            for k in KS:
                c.check(k, ("rotated", "scan_small", small, "nq", nq), q=raw, nq=nq, q_rot=q_rot, tag="rot-nq%d" % nq, rotate=True)
    finally:
        c.close()


@pytest.mark.parametrize("k", [129, 2048])
@pytest.mark.parametrize("name", BIGK_CASES)
def test_big_k_filter_scan(amd, orc, name, k):
    """launch_adc_scan_bigk (k = 129 .. 2048 on >= 65 536 rows with 8 k <= rows): sampled histogram bound, candidate lists, the exact
    kernel behind it for the queries it flags.  Not observable from outside: "scan_bigk" 1 and 0 must each give the oracle's lists."""
    c = Case(amd, orc, name, rows=sc.ROWS_BIG)
    assert k * 8 <= sc.ROWS_BIG
    try:
        for bigk in (1, 0):
            with sc.tuning(amd, scan_bigk=bigk):
                c.check(k, ("scan_bigk", bigk))
    finally:
        c.close()
