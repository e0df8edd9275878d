"""CPU: orc_hnsw_search against the reference's own searchKnn (oracle/_ref/libref_hnsw.so) on the shapes the golden graphs
lack -- the specification tests/test_gpu_hnsw_edges.py leans on: IP with D % 4 != 0, L2 with D % 4 == 0 and D % 16 != 0,
level-0 lists longer than 64, labels that are not monotone in the internal id over duplicated rows, graphs smaller than k,
and queries that are not finite."""
import os

import numpy as np
import pytest

from conftest import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_REF = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libref_hnsw.so"))
pytestmark = pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/libref_hnsw.so not built")
GRID = ((1, 1), (10, 10), (10, 50), (50, 20), (100, 300))


def quarter_rows(n, D, seed, dup=200):
    """coordinates rounded to quarters and `dup` rows repeated: equal distances everywhere, the heaps decide"""
    rng = np.random.default_rng(seed)
    x = np.round(rng.normal(size=(n, D)) * 4).astype(np.float32) / 4
    if n >= 2 * dup:
        x[n // 2:n // 2 + dup] = x[:dup]
    return x


def scattered_labels(n, seed):
    """distinct labels in no order, some above 2^32 (below 2^63: the reference compares them as size_t)"""
    rng = np.random.default_rng(seed)
    lab = rng.choice(1 << 20, size=n, replace=False).astype(np.int64)
    lab[rng.random(n) < 0.3] += np.int64(1) << 40
    return lab


def odd_queries(x, seed, nq=24):
    """database rows, perturbed rows, then the non-finite ones and the all-zero query"""
    rng = np.random.default_rng(seed)
    n, D = x.shape
    q = x[rng.integers(0, n, nq)].copy()
    q[nq // 2:] += rng.normal(size=(nq - nq // 2, D)).astype(np.float32)
    odd = x[rng.integers(0, n, 7)].copy()
    odd[0, D // 2] = np.nan
    odd[1, 0] = np.inf
    odd[2, D - 1] = -np.inf
    odd[3] = 0.0
    odd[4, :] = np.nan
    odd[5, 0], odd[5, D - 1] = np.inf, -np.inf
    odd[6, D // 2] = -np.nan
    return np.ascontiguousarray(np.concatenate([q, odd]), np.float32)


CASES = {
    # name: (metric, D, n, M, efc, scattered labels)
    "ip10": (0, 10, 2000, 8, 40, False),
    "l2f20": (1, 20, 2000, 8, 40, False),
    "l2_m40": (1, 8, 3000, 40, 100, False),
    "ip_m40": (0, 12, 3000, 40, 100, True),
    "dups_ip": (0, 16, 2000, 8, 40, True),
    "dups_l2": (1, 7, 2000, 8, 40, True),
    "n1": (1, 12, 1, 8, 40, False),
    "n2": (0, 10, 2, 8, 40, True),
    "n5": (1, 20, 5, 8, 40, True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_oracle_hnsw_search_matches_reference_on_edge_shapes(orc, tmp_path, case):
    """Labels and distance bits of orc.hnsw_search equal RefHnsw().search on a graph the reference has just built, for every
    (k, ef) of the GPU suite's grid.  The non-finite queries stay in: the reference's answer for them is reproducible (asked
    twice here, same bytes) -- every comparison of its heaps is a deterministic function of the bits, NaN included -- and
    the oracle restates those heaps, the (distance, label) result queue among them, comparison for comparison."""
    from oracle import binding as ob
    metric, D, n, M, efc, scattered = CASES[case]
    x = quarter_rows(n, D, 500 + D + M)
    if case.startswith("dups"):
        x[100:500] = np.repeat(x[100:150], 8, axis=0)          # 50 groups of 8 identical rows
    labels = scattered_labels(n, 7) if scattered else None
    path = str(tmp_path / "g.hnsw")
    rh = ob.RefHnsw()
    rh.build(metric, x, path, M, efc, labels=labels)
    blob = open(path, "rb").read()
    q = odd_queries(x, 11)
    if case.startswith("dups"):
        q = np.ascontiguousarray(np.concatenate([x[100:500:8], q]))
    for k, ef in GRID:
        rd, rl = rh.search(metric, D, path, q, k, ef)
        rd2, rl2 = rh.search(metric, D, path, q, k, ef)
        assert np.array_equal(rl, rl2) and np.array_equal(bits(rd), bits(rd2)), (case, k, ef, "reference not reproducible")
        od, ol = orc.hnsw_search(blob, metric, D, q, k, ef)
        bad = [i for i in range(len(q)) if not (np.array_equal(ol[i], rl[i]) and np.array_equal(bits(od[i]), bits(rd[i])))]
        assert not bad, (case, k, ef, bad, ol[bad[0]][:8], rl[bad[0]][:8], od[bad[0]][:8], rd[bad[0]][:8])
        if n < k:
            assert (ol[:, n:] == -1).all() and not bits(od[:, n:]).any()
