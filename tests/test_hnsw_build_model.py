"""CPU: tests/hnsw_build_model.py (the batch-synchronous HNSW build of DESIGN 4.11, restated in Python) against bytes that others
wrote, before test_gpu_hnsw_build_batches.py holds the kernels to it.

  * max_batch = 1 is the reference's sequential insertion: the model rebuilds the five golden graphs byte for byte from the rows,
    labels and levels parsed out of the golden files themselves -- search, heuristic, heap layouts, stale words and file writer.
  * the same against the host mirror's sequential file (the hnsw_build CLI) on tie-heavy rows, both metrics, one D % 4 != 0.
  * the numpy distances the larger shapes use are the oracle's, bit for bit, for every (metric, D) they are used at.
  * every shape of the shared table reaches the batch-only path it is there for: asserted from the model's counters."""
import numpy as np
import pytest

import hnsw_build_model as hm
from conftest import bits
from test_gpu_hnsw_build import CASES as GOLDEN, host_build, parse, tie_heavy


@pytest.mark.parametrize("case", GOLDEN)
def test_sequential_model_rebuilds_golden_graph(orc, golden, case):
    g = golden.hnsw
    blob = g[case + "_index"]
    metric, D, n, M, efc, k, ef = (int(v) for v in g[case + "_meta"])
    p = parse(blob)
    for vectorised in (False, True):
        out, cnt = hm.build_model(orc, p["rows"], metric, M, efc, p["levels"], p["labels"], 1, vectorised=vectorised)
        out = np.frombuffer(out, dtype=np.uint8)
        assert out.size == blob.size and np.array_equal(out, blob), (case, vectorised, hm.first_difference(parse(out), p, cnt))
        assert cnt["largest_batch"] == 1 and cnt["batches"] == n and cnt["props_target"] <= p["levels"].max() + 1


@pytest.mark.parametrize("metric,D,n,M,efc", [(0, 20, 700, 8, 40), (1, 16, 700, 5, 30), (1, 7, 600, 4, 20), (0, 10, 500, 24, 30)])
def test_sequential_model_matches_host_mirror(orc, tmp_path, metric, D, n, M, efc):
    x = tie_heavy(n, D, 300 + D)
    seq = host_build(tmp_path, x, metric, M, efc, "seq")
    p = parse(seq)
    out, cnt = hm.build_model(orc, x, metric, M, efc, p["levels"], None, 1)
    out = np.frombuffer(out, dtype=np.uint8)
    assert out.size == seq.size and np.array_equal(out, seq), hm.first_difference(parse(out), p, cnt)
    assert cnt["tie_runs"] >= 1     # duplicated rows: the tie order of queue_closest decided something


def test_numpy_distances_are_the_oracles(orc, golden):
    """dist_row against orc.dist(metric, 4, ., .) in both argument orders: every width of the table, of the golden graphs and of
    the host-mirror shapes above; tie-heavy rows (exact zeros and duplicates) and plain normal ones"""
    widths = {(c["metric"], c["rows"]().shape[1]) for c in hm.CASES.values()}
    widths |= {(int(golden.hnsw[c + "_meta"][0]), int(golden.hnsw[c + "_meta"][1])) for c in GOLDEN}
    widths |= {(0, 20), (1, 16), (1, 7), (0, 10)}
    rng = np.random.default_rng(3)
    for metric, D in sorted(widths):
        x = np.concatenate([tie_heavy(420, D, D), rng.normal(size=(60, D)).astype(np.float32) * 3]).astype(np.float32)
        for i in (0, 7, 211, 450):
            got = hm.dist_row(x, metric, i)
            assert got.dtype == np.float32
            fwd = np.array([orc.dist(metric, 4, x[i], x[j]) for j in range(x.shape[0])], np.float32)
            back = np.array([orc.dist(metric, 4, x[j], x[i]) for j in range(x.shape[0])], np.float32)
            assert np.array_equal(bits(got), bits(fwd)) and np.array_equal(bits(got), bits(back)), (metric, D, i)


def test_schedule():
    lv = [1, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0]
    # frac 1: batches double; row 4 raises the top level by two and ends its batch, the next batch enters from it
    assert hm.schedule(lv, 12, 0, 1, 8192) == [(1, 2, 0, 1, False), (2, 4, 0, 1, False), (4, 5, 0, 1, True), (5, 10, 4, 3, False),
                                                (10, 12, 4, 3, False)]
    assert [b[:2] for b in hm.schedule(lv, 12, 3, 1, 8192)] == [(1, 2), (2, 4), (4, 5), (5, 8), (8, 11), (11, 12)]
    assert [b[:2] for b in hm.schedule(lv, 12, 0, 1, 2)] == [(1, 2), (2, 4), (4, 5), (5, 7), (7, 9), (9, 11), (11, 12)]
    assert [b[:2] for b in hm.schedule(lv, 12, 0, 32, 8192)] == [(i, i + 1) for i in range(1, 12)]
    assert hm.schedule([2], 1, 0) == []


_built = {}


def model_of(orc, tmp_path, name):
    """(rows, labels, the host mirror's sequential file parsed, the model's file, counters) of one shape of the table, built once"""
    if name not in _built:
        c = hm.CASES[name]
        x = c["rows"]()
        labels = c["labels"](x.shape[0]) if "labels" in c else None
        blob = host_build(tmp_path, x, c["metric"], c["M"], c["efc"], "lv_" + name)
        seq = parse(blob)
        seq["header"] = blob[:96].tobytes()
        out, cnt = hm.build_model(orc, x, c["metric"], c["M"], c["efc"], seq["levels"], labels, c["max_batch"], c.get("frac", 32),
                                  vectorised=True)
        _built[name] = (x, labels, seq, out, cnt)
    return _built[name]


@pytest.mark.parametrize("name", list(hm.CASES))
def test_case_reaches_its_path(orc, tmp_path, name):
    x, labels, seq, out, cnt = model_of(orc, tmp_path, name)
    print(name, {k: v for k, v in cnt.items() if k != "touched"})
    assert hm.CASES[name]["need"](cnt), {k: v for k, v in cnt.items() if k != "touched"}
    g = parse(out)
    assert np.array_equal(g["levels"], seq["levels"]) and g["ep"] == seq["ep"] and out[:96] == seq["header"]
    if name == "G":
        d = hm.dist_row(x, 0, 0)
        assert len(set(bits(d).tolist())) == 1
    if name == "F-rise2":   # the file's own levels say the same as the counters: some row rises two levels over everything before it
        lv = seq["levels"]
        assert any(lv[i] >= lv[:i].max() + 2 for i in range(1, len(lv)))
