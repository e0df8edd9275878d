"""GPU: cvtmi_hnsw_add (csrc/api_hnsw.hip, csrc/hnsw_build.hip started from a graph that holds rows), DESIGN 4.11.1.

Every test compares whole files or whole result arrays, without a tolerance:
  * max_batch = 1 is the reference's sequential addPoint: build of a prefix + adds of the rest rebuild the golden graphs (and, where
    oracle/_ref is built, the reference's fresh file of tie-heavy rows); load + add writes what the host mirror's loadIndex + addPoint
    loop writes (tests/test_host_hnsw_add.py pins that loop to the reference's files), with spare capacity, without, and from an
    empty file;
  * larger batches: build(x[:n0], b) + add(x[n0:], b) is build(x, b) at a batch boundary n0, and off a boundary it is the file of
    tests/hnsw_build_model.py under the schedule "the build's up to n0, then the rule restarted at n0";
  * a handle whose scratch sets were planned for 33 nodes answers on 3000 exactly as a fresh handle of the same file does."""
import numpy as np
import pytest

import hnsw_build_model as hm
from conftest import bits
from test_gpu_hnsw import opq_over_graph
from test_gpu_hnsw_build import CASES as GOLDEN, HAVE_REF, assert_sound, host_build, parse, tie_heavy
from test_gpu_hnsw_build_batches import explain, model_of
from test_gpu_hnsw_edges import mixed_queries, same
from test_host_hnsw_add import build_then_add_schedule, empty_index, host_add, with_capacity

pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available()
    import cvt_amd
    return cvt_amd


def saved(idx):
    return np.frombuffer(idx.save(), dtype=np.uint8)


def add_in_calls(idx, x, labels, n0, max_batch):
    """the rows from n0 on in several calls: one of a single row, one of no rows, one of up to 50, one of the rest; returns the
    (first, end) of the last call that held rows"""
    n = x.shape[0]
    cuts = [n0, min(n0 + 1, n), min(n0 + 1, n), min(n0 + 51, n), n]
    last = None
    for s, e in zip(cuts, cuts[1:]):
        before = idx.ntotal
        idx.add(x[s:e], None if labels is None else labels[s:e], max_batch=max_batch)
        assert idx.ntotal == before + (e - s) == e
        if e > s:
            last = (s, e)
            assert idx.last_add()[0] == s
    return last


# ---- 1. sequential: the reference's addPoint -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0", [1, 33])
@pytest.mark.parametrize("case", GOLDEN)
def test_sequential_adds_rebuild_golden_graph(amd, golden, case, n0):
    g = golden.hnsw
    blob = g[case + "_index"]
    metric, D, n, M, efc, k, ef = (int(v) for v in g[case + "_meta"])
    p = parse(blob)
    idx = amd.hnsw_build(p["rows"][:n0], metric, M, efc, labels=p["labels"][:n0], max_batch=1)
    assert idx.level_draws() == n0
    s, e = add_in_calls(idx, p["rows"], p["labels"], n0, 1)
    assert idx.level_draws() == n
    out = saved(idx)
    assert out.size == blob.size and np.array_equal(out, blob)
    assert idx.last_add() == (s, e - s, 1, n)


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref not built (needs the reference tree at build time)")
def test_sequential_adds_match_reference(amd, tmp_path):
    from oracle import binding as ob
    metric, D, n, M, efc = 0, 20, 3000, 24, 50
    x = tie_heavy(n, D, 1000 + D)
    path = str(tmp_path / "ref.hnsw")
    ob.RefHnsw().build(metric, x, path, M, efc, threads=1)
    ref = np.fromfile(path, dtype=np.uint8)
    idx = amd.hnsw_build(x[:33], metric, M, efc, max_batch=1)
    add_in_calls(idx, x, None, 33, 1)
    out = saved(idx)
    assert out.size == ref.size and np.array_equal(out, ref)


# ---- 2. load + add: the mirror's loadIndex + addPoint loop -----------------------------------------------------------------------------
def test_load_then_add_is_the_host_loop(amd, tmp_path, golden):
    g = golden.hnsw
    blob = g["l2f16_index"]
    metric, D, n, M, efc, k, ef = (int(v) for v in g["l2f16_meta"])
    rng = np.random.default_rng(16)
    extra = rng.normal(size=(40, D)).astype(np.float32)
    extra[7] = parse(blob)["rows"][3]                       # a row the graph already holds: a second node, distance 0
    labels = np.arange(40, dtype=np.uint64) * 5 + 100000
    labels[9] = parse(blob)["labels"][0]                    # a repeated label gets a second node
    # as loaded (no spare capacity), with spare capacity that the rows fit into, with spare capacity that they exceed
    for tag, cap, cap_after in (("tight", n, n + 40), ("fits", n + 50, n + 50), ("exceeds", n + 10, n + 40)):
        src = with_capacity(blob, cap)
        idx = amd.HnswIndex(src.tobytes(), metric, D)
        assert idx.level_draws() == 0 and np.array_equal(saved(idx), src)
        idx.add(extra[:25], labels[:25], max_batch=1)
        idx.add(extra[25:], labels[25:], max_batch=1)
        assert idx.level_draws() == 40 and idx.ntotal == n + 40
        out = saved(idx)
        want = host_add(tmp_path, src, extra, D, metric, tag, labels=labels)
        assert parse(out)["cap"] == cap_after == parse(want)["cap"] == idx.last_add()[3]
        assert out.size == want.size and np.array_equal(out, want), tag
    # default labels are the internal ids; reserve raises max_elements and never lowers it
    idx = amd.HnswIndex(blob.tobytes(), metric, D)
    idx.reserve(n + 7)
    idx.reserve(n - 5)
    assert np.array_equal(saved(idx), with_capacity(blob, n + 7))
    idx.add(extra[:5], max_batch=1)
    want = host_add(tmp_path, with_capacity(blob, n + 7), extra[:5], D, metric, "ids")
    assert np.array_equal(saved(idx), want) and parse(want)["cap"] == n + 7
    assert np.array_equal(parse(want)["labels"][n:], np.arange(n, n + 5, dtype=np.uint64))


@pytest.mark.parametrize("metric,D,M,efc", [(1, 16, 8, 40), (0, 10, 5, 3)])
def test_add_to_an_empty_file(amd, tmp_path, metric, D, M, efc):
    """cur_element_count = 0, maxlevel = -1: row 0 seeds alone, the capacity of 5 is exceeded, and the result is a plain build"""
    x = tie_heavy(400, D, 50 + D)
    src = empty_index(D, M, efc, 5)
    idx = amd.HnswIndex(src.tobytes(), metric, D)
    assert idx.ntotal == 0 and idx.level_draws() == 0 and np.array_equal(saved(idx), src)
    idx.add(x[:1], max_batch=1)
    assert idx.last_add() == (0, 1, 1, 5)
    idx.add(x[1:], max_batch=1)
    out = saved(idx)
    want = host_add(tmp_path, src, x, D, metric, "empty")
    assert np.array_equal(out, want)
    assert np.array_equal(out, host_build(tmp_path, x, metric, M, efc, "plain"))
    assert idx.level_draws() == 400 and idx.last_add()[3] == 400
    # and in one call on another empty handle, default schedule: the build's own file
    idx = amd.HnswIndex(src.tobytes(), metric, D)
    idx.add(x)
    assert np.array_equal(saved(idx), saved(amd.hnsw_build(x, metric, M, efc, max_batch=0)))


# ---- 3. batches: a boundary of the build's schedule ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A-7", "F", "G"])
def test_build_plus_add_at_a_batch_boundary_is_the_build(amd, orc, tmp_path, name):
    c = hm.CASES[name]
    x, labels, want, cnt = model_of(orc, tmp_path, name)
    n = x.shape[0]
    frac, b = c.get("frac", 32), c["max_batch"]
    sched = hm.schedule(parse(want)["levels"], n, b, frac)
    n0 = sched[len(sched) // 2][0]
    assert 1 < n0 < n
    try:
        amd.set_tuning("hnsw_build_frac", frac)
        amd.set_tuning("hnsw_build_cap", 8192)
        idx = amd.hnsw_build(x[:n0], c["metric"], c["M"], c["efc"], labels=None if labels is None else labels[:n0], max_batch=b)
        idx.add(x[n0:], None if labels is None else labels[n0:], max_batch=b)
        got = saved(idx)
        first, batches, largest, cap = idx.last_add()
        print("%s: n0 = %d of %d, add in %d batches (largest %d)" % (name, n0, n, batches, largest))
        assert np.array_equal(got, want), explain(got, want, cnt)
        assert np.array_equal(got, saved(amd.hnsw_build(x, c["metric"], c["M"], c["efc"], labels=labels, max_batch=b)))
        assert first == n0 and batches == len(sched) - len(sched) // 2 and batches > 1 and largest > 1 and cap == n
        assert largest == max(e - s for s, e, _, _, _ in sched[len(sched) // 2:])
    finally:
        amd.set_tuning("hnsw_build_frac", 32)
        amd.set_tuning("hnsw_build_cap", 8192)


# ---- 4. batches: off a boundary, against the model -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A-7", "C", "F-rise2"])
def test_add_off_a_boundary_is_the_model(amd, orc, tmp_path, monkeypatch, name):
    import torch
    c = hm.CASES[name]
    x = c["rows"]()
    n = x.shape[0]
    frac, b = c.get("frac", 32), c["max_batch"]
    levels = parse(host_build(tmp_path, x, c["metric"], c["M"], c["efc"], "seq_" + name))["levels"]
    sched = hm.schedule(levels, n, b, frac)
    if name == "F-rise2":
        n0 = 100           # row 115 rises two levels: in the build it ends a batch of three early, here the batch it opens
        assert levels[115] >= levels[:115].max() + 2
    else:
        s, e = next((s, e) for s, e, _, _, _ in sched[len(sched) // 2:] if e - s > 1)
        n0 = s + 1
    assert n0 not in [s for s, _, _, _, _ in sched] and 1 < n0 < n
    patched = build_then_add_schedule(n0, b, b)
    plan = patched(levels, n, b, frac)
    assert plan != sched and n0 in [s for s, _, _, _, _ in plan]
    if name == "F-rise2":
        assert any(s <= 115 and e == 116 and cut for s, e, _, _, cut in plan)
    monkeypatch.setattr(hm, "schedule", patched)
    want, cnt = hm.build_model(orc, x, c["metric"], c["M"], c["efc"], levels, None, b, frac, vectorised=True)
    want = np.frombuffer(want, dtype=np.uint8)
    try:
        amd.set_tuning("hnsw_build_frac", frac)
        amd.set_tuning("hnsw_build_cap", 8192)
        idx = amd.hnsw_build(x[:n0], c["metric"], c["M"], c["efc"], max_batch=b)
        idx.add(x[n0:], max_batch=b)
        got = saved(idx)
        print("%s: n0 = %d of %d, add in %d batches (largest %d)" % ((name, n0, n) + idx.last_add()[1:3]))
        assert np.array_equal(got, want), explain(got, want, cnt)
        assert idx.last_add()[1] == len([p for p in plan if p[0] >= n0])
        if name == "A-7":   # device rows on a side stream
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                xd = torch.from_numpy(x).cuda()
                idx = amd.hnsw_build(xd[:n0].contiguous(), c["metric"], c["M"], c["efc"], max_batch=b)
                idx.add(xd[n0:].contiguous(), max_batch=b)
            s.synchronize()
            got = saved(idx)
            assert np.array_equal(got, want), explain(got, want, cnt)
    finally:
        amd.set_tuning("hnsw_build_frac", 32)
        amd.set_tuning("hnsw_build_cap", 8192)


# ---- 5. scratch planned for a smaller graph --------------------------------------------------------------------------------------------
def test_searches_after_growth_use_scratch_for_the_grown_graph(amd, orc):
    import cvt_amd.capi as capi
    metric, D, M, efc, n0, n = 1, 16, 8, 40, 33, 3000
    x = tie_heavy(n, D, 333)
    labels = np.arange(n, dtype=np.uint64) * 3 + 11
    q = mixed_queries(x, 48, 5)
    idx = amd.hnsw_build(x[:n0], metric, M, efc, labels=labels[:n0], max_batch=1)
    small = np.full(1, ~np.uint64(0), np.uint64)
    same(idx.search_masked(q, 10, 50, small), idx.search(q, 10, 50), "33 nodes")      # scratch sets planned for 33 nodes exist now
    idx.add(x[n0:1000], labels[n0:1000])
    idx.add(x[1000:], labels[1000:])
    assert idx.ntotal == n and idx.last_add()[2] > 1
    blob = idx.save()
    assert_sound(parse(blob))
    fresh = amd.HnswIndex(blob, metric, D)
    ones = np.full((n + 63) // 64, ~np.uint64(0), np.uint64)
    for k, ef in ((10, 50), (100, 300), (1, 1)):
        want = fresh.search(q, k, ef)
        same(idx.search(q, k, ef), want, ("grown", k, ef))
        same(idx.search_masked(q, k, ef, ones), want, ("grown, all-ones", k, ef))
        same(fresh.search_masked(q, k, ef, ones), want, ("fresh, all-ones", k, ef))
    assert (np.asarray(idx.search(q, 10, 50)[1]) >= labels[n0]).any()                 # added rows are found
    with pytest.raises(capi.CvtmiError) as e:
        idx.search_masked(q, 10, 50, small)
    assert e.value.code == EINVAL
    m = idx.mask_from_labels(labels[[2500]])
    assert m.shape[0] == ones.shape[0] and int(m[2500 >> 6]) == 1 << (2500 & 63) and not np.delete(m, 2500 >> 6).any()
    # an OPQ index that still holds the 33 code rows of the graph before it grew: refused until the caller appends the rest
    full, books, codes, _, _, mk = opq_over_graph(amd, orc, blob, D, 8, 64)
    opq = mk(books)
    opq.add_codes(codes[:n0])
    with pytest.raises(capi.CvtmiError) as e:
        idx.search_adc(opq, q, 10, 50)
    assert e.value.code == EINVAL and "code rows" in str(e.value)
    opq.add_codes(codes[n0:])
    want = fresh.search_adc(full, q, 10, 50)
    same(idx.search_adc(opq, q, 10, 50), want, "adc")
    same(idx.search_adc_masked(opq, q, 10, 50, ones), want, "adc, all-ones")
    opq.close()
    full.close()


# ---- 6. the hnsw_add CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_gpu_mode(amd, tmp_path, golden):
    g = golden.hnsw
    blob = g["ip20_index"]
    metric, D, n, M, efc, k, ef = (int(v) for v in g["ip20_meta"])
    extra = tie_heavy(400, D, 20)
    labels = np.arange(400, dtype=np.uint64) + 10 ** 6
    host = host_add(tmp_path, blob, extra, D, metric, "host", labels=labels)
    seq = host_add(tmp_path, blob, extra, D, metric, "gpu1", labels=labels, mode="gpu:1")
    assert np.array_equal(seq, host)
    dflt = parse(host_add(tmp_path, blob, extra, D, metric, "gpu", labels=labels, mode="gpu"))
    assert_sound(dflt)
    h = parse(host)
    assert dflt["cnt"] == n + 400 == dflt["cap"] and dflt["sizes"] == h["sizes"] and np.array_equal(dflt["labels"], h["labels"])
    assert np.array_equal(bits(dflt["rows"]), bits(h["rows"]))
    # cont: the stream continues the build that wrote the index, on the device copy as on the host
    a = host_add(tmp_path, blob, extra, D, metric, "host_cont", labels=labels, cont=True)
    b = host_add(tmp_path, blob, extra, D, metric, "gpu1_cont", labels=labels, mode="gpu:1", cont=True)
    assert np.array_equal(a, b) and not np.array_equal(a, host)
