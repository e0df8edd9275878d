"""CPU: orc_topk_pairs (the checker of cvtmi_topk_select and of the video ranking) against the reference's own get_sort_results
run live (oracle/_ref/libref_opq.so): std::partial_sort_copy over (float, uint) pairs, where -0.0 and +0.0 are equal and tie by
index.  Finite, signed-zero, infinite and tie-heavy scores, k below and above the number of scores (the reference returns k pairs,
(0, 0) past the end).  NaN is left out: the pairs are then not ordered and neither side's result is specified."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import bits

from oracle import binding as ob

pytestmark = pytest.mark.skipif(not ob.ref_available(), reason="oracle/_ref not built")


def ref_sort_results(score, k):
    lib = C.CDLL(os.path.join(os.path.dirname(ob.__file__), "_ref", "libref_opq.so"))
    score = np.ascontiguousarray(score, np.float32)
    d = np.full(k, np.nan, np.float32); i = np.full(k, 0xFFFFFFFF, np.uint32)
    lib.ref_sort_results(C.c_void_p(score.ctypes.data), C.c_int(score.size), C.c_int(k), C.c_void_p(d.ctypes.data),
                         C.c_void_p(i.ctypes.data))
    return d, i.astype(np.int64)


def _scores(kind, n, rng):
    if kind == "random":
        return rng.normal(size=n).astype(np.float32)
    if kind == "ties":
        return rng.integers(0, 4, size=n).astype(np.float32)
    if kind == "zeros":                           # {+0, -0, +0, -0, ...} and a few values around them
        x = np.where(np.arange(n) % 2 == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        x[rng.random(n) < 0.1] = 1.0
        x[rng.random(n) < 0.1] = -1.0
        return x
    if kind == "specials":
        pool = np.array([np.inf, -np.inf, 0.0, -0.0, 3.4028235e38, -3.4028235e38, 1e-45, -1e-45, 1.0, 1.0, 2.0], np.float32)
        return pool[rng.integers(0, pool.size, size=n)]
    if kind == "clamp":                           # the video scores of a query: most videos at the 1.0 clamp
        x = np.ones(n, np.float32)
        x[rng.random(n) < 0.2] = rng.uniform(0, 1, size=1).astype(np.float32)[0]
        return x
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["random", "ties", "zeros", "specials", "clamp"])
def test_topk_pairs_matches_reference(orc, kind):
    rng = np.random.default_rng(len(kind))
    for n in (1, 4, 5, 37, 1000):
        x = _scores(kind, n, rng)
        for k in sorted({1, 3, n - 1, n, n + 1, 2 * n + 3} - {0}):
            rd, ri = ref_sort_results(x, k)
            od, oi = orc.topk_pairs(x, k)
            m = min(k, n)
            assert od.size == m
            assert np.array_equal(oi, ri[:m]), (kind, n, k)
            assert np.array_equal(bits(od), bits(rd[:m])), (kind, n, k)      # a -0.0 keeps its sign on both sides
            assert np.all(ri[m:] == 0) and np.all(bits(rd[m:]) == 0)          # value-initialised pairs past the end


def test_signed_zeros_tie_by_index(orc):
    """the case the device kernel once got wrong: {+0, -0, +0, -0}, k = 4 -> indices 0 1 2 3"""
    x = np.array([0.0, -0.0, 0.0, -0.0], np.float32)
    rd, ri = ref_sort_results(x, 4)
    assert ri.tolist() == [0, 1, 2, 3]
    assert bits(rd).tolist() == [0, 0x80000000, 0, 0x80000000]
    od, oi = orc.topk_pairs(x, 4)
    assert oi.tolist() == [0, 1, 2, 3] and np.array_equal(bits(od), bits(rd))
