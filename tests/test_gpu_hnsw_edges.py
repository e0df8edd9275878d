"""GPU: the batched HNSW search (csrc/hnsw.hip, hnsw_heap.h) on every distance instantiation, on neighbour lists longer than a
wave, with the LDS / HBM split of both queues moved across ef, with many queries per slot, with labels that are not monotone in
the internal id over duplicated rows, with queries that are not finite, and on graphs smaller than k.

Every assertion is the same: labels equal and distance BITS equal to the oracle's traversal (oracle/cvt_oracle.c, pinned to the
reference's own searchKnn on these shapes by tests/test_oracle_hnsw_edges.py) of the same index bytes, queries, k and ef.  Rows
are quantised to quarters and partly repeated wherever a section allows it, so equal distances are common and the answer is
decided by the heap mechanics, not by the arithmetic alone."""
import numpy as np
import pytest

from conftest import bits
from test_gpu_hnsw import check_search_adc, check_search_adc_rerank, opq_over_graph
from test_gpu_hnsw_build import host_build, parse, tie_heavy
from test_oracle_hnsw_edges import GRID, odd_queries, quarter_rows, scattered_labels

pytestmark = pytest.mark.gpu
TOP_LDS = (0, 16, 17, 64, 255, 256, 257)
EFS = (15, 16, 17, 63, 64, 65, 254, 255, 256, 257, 511, 1023, 1024)
K_IS_EF = (16, 256, 1024)


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()
    return cvt_amd


def same(got, want, tag):
    """labels equal; distance bits equal wherever the distance is a number, and a NaN where the oracle has a NaN.  The sign and
    payload of a NaN are no part of the answer: they belong to the instruction set that made it (0 x inf is 0xffc00000 on the
    x86 host the oracle and the reference run on and 0x7fc00000 on gfx950; which operand's payload an addition of two NaNs
    keeps, and whether 1 - NaN is done as a negation, is the compiler's choice on both), and they never reach a comparison."""
    d, lab = (np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v) for v in got)
    assert np.array_equal(lab, want[1]), tag
    nan = np.isnan(want[0])
    assert np.array_equal(np.isnan(d), nan), tag
    assert np.array_equal(bits(np.where(nan, 0, d)), bits(np.where(nan, 0, want[0]))), tag


def mixed_queries(x, nq, seed):
    """half of them database rows (distance 0 to every copy of the row), half perturbed rows"""
    rng = np.random.default_rng(seed)
    q = x[rng.integers(0, x.shape[0], nq)].copy()
    q[nq // 2:] += rng.normal(size=(nq - nq // 2, x.shape[1])).astype(np.float32)
    return np.ascontiguousarray(q, np.float32)


def pq_layouts(D):
    """(M, K) of the ADC searches run over a D-dimensional graph: every M of {16, 8, 4} that divides D"""
    return [(M, 64 if M == 8 else 256) for M in (16, 8, 4) if D % M == 0]


# ---- 1. every distance variant: plain, ADC and re-rank ------------------------------------------------------------------------------
# launch_hnsw_search / launch_hnsw_rerank: IP, D % 4 != 0 -> <true, 1>; IP, D % 4 == 0 -> <true, 4>; L2, D % 4 != 0 -> <false, 1>;
# L2, D % 4 == 0 and D % 16 != 0 -> <false, 4>; L2, D % 16 == 0 -> <false, 8>
@pytest.mark.parametrize("metric,D", [(0, 10), (0, 33), (0, 20), (0, 128), (1, 7), (1, 12), (1, 20), (1, 100), (1, 16), (1, 64)])
def test_every_distance_variant(amd, orc, metric, D):
    x = tie_heavy(3000, D, 2000 + D)
    ix = amd.hnsw_build(x, metric, 8, 40, max_batch=1)
    blob = ix.save()
    q = mixed_queries(x, 64, D)
    for k, ef in GRID:
        same(ix.search(q, k, ef), orc.hnsw_search(blob, metric, D, q, k, ef), (metric, D, k, ef))
    for M, K in pq_layouts(D):
        opq, books, ocodes, rot, xv, _ = opq_over_graph(amd, orc, blob, D, M, K)
        assert np.array_equal(bits(xv), bits(x))
        check_search_adc(amd, orc, ix, opq, blob, books, ocodes, rot, q, GRID, (metric, D, M))
        check_search_adc_rerank(orc, ix, opq, blob, metric, D, books, ocodes, rot, xv, q, ((5, 40, 40), (10, 64, 30), (1, 16, 8)),
                                (metric, D, M))
        opq.close()
    ix.close()


# ---- 2. neighbour lists longer than 64 ----------------------------------------------------------------------------------------------
# The GPU builder stops at M = 32; the host mirror's hnsw_build CLI (pinned to the reference at M = 48 by test_host_hnsw_build.py)
# has no such limit.  Rows are i.i.d. normal and high-dimensional: in clustered or low-dimensional rows getNeighborsByHeuristic2
# prunes nearly every list far below maxM0 (measured: 20 - 75 lists over 64 links among 4000 clustered rows, against 380 - 570
# here), and a test over those would run the second trip a handful of times.
WIDE = {"l2_m40": (1, 128, 6000, 40), "l2_m48": (1, 128, 6000, 48), "ip_m40": (0, 64, 4000, 40), "ip_m48": (0, 64, 4000, 48)}


@pytest.mark.parametrize("case", list(WIDE))
def test_level0_lists_longer_than_a_wave(amd, orc, tmp_path, case):
    metric, D, n, M = WIDE[case]
    x = np.random.default_rng(40 + M + metric).normal(size=(n, D)).astype(np.float32)
    blob = host_build(tmp_path, x, metric, M, 100, case)
    g = parse(blob)
    wide = int((g["l0"][:, 0] > 64).sum())
    print("%s: %d of %d level-0 lists hold more than 64 links (longest %d)" % (case, wide, n, g["l0"][:, 0].max()))
    assert g["maxM0"] == 2 * M and wide >= 200
    blob = blob.tobytes()
    ix = amd.HnswIndex(blob, metric, D)
    q = mixed_queries(x, 64, M)
    for k, ef in GRID:
        same(ix.search(q, k, ef), orc.hnsw_search(blob, metric, D, q, k, ef), (case, k, ef))
    opq, books, ocodes, rot, _, _ = opq_over_graph(amd, orc, blob, D, 16, 256)
    check_search_adc(amd, orc, ix, opq, blob, books, ocodes, rot, q, ((10, 50), (100, 300)), case)


def upper_walk(g, dq):
    """the greedy descent of searchKnn (hnswalg.h:692-712) over a parsed file, dq = the query's distance to every node: returns the
    level-0 entry node, the number of expanded lists with more than 64 links, and how often the minimum moved to a neighbour in
    position 64 or later of such a list"""
    cur, curdist, wide, late = g["ep"], dq[g["ep"]], 0, 0
    for level in range(g["maxlevel"], 0, -1):
        changed = True
        while changed:
            changed = False
            u = g["upper"][(cur, level)]
            size = int(u[0])
            wide += size > 64
            for j in range(size):
                c = int(u[1 + j])
                if dq[c] < curdist:
                    curdist, cur, changed = dq[c], c, True
                    late += j >= 64
    return cur, wide, late


def test_upper_lists_longer_than_a_wave(amd, orc, tmp_path):
    """M = 72: levels >= 1 hold n / 72 nodes, and the pruning heuristic leaves a list there above 64 links only for a node that
    beats its neighbours' mutual distances -- under the inner product, a row of large norm.  Norms are log-normal, so a few
    hundredths of the upper nodes are such hubs, and they are the nodes every descent passes through."""
    rng = np.random.default_rng(72)
    n, D, M = 30000, 8, 72
    x = (rng.normal(size=(n, D)) * np.exp(rng.normal(size=(n, 1)))).astype(np.float32)
    blob = host_build(tmp_path, x, 0, M, 100, "m72")
    g = parse(blob)
    up = [int(u[0]) for u in g["upper"].values()]
    print("M = 72: %d of %d upper lists hold more than 64 links; %d level-0 lists more than 64, %d more than 128"
          % (sum(c > 64 for c in up), len(up), int((g["l0"][:, 0] > 64).sum()), int((g["l0"][:, 0] > 128).sum())))
    assert sum(c > 64 for c in up) >= 5
    q = np.ascontiguousarray(np.concatenate([mixed_queries(x, 96, 1), rng.normal(size=(160, D)).astype(np.float32)]))
    nodes = sorted({i for i, _ in g["upper"]})
    walks = [upper_walk(g, {i: orc.dist(0, 4, qi, x[i]) for i in nodes}) for qi in q]
    through, late = sum(w[1] > 0 for w in walks), sum(w[2] > 0 for w in walks)
    print("M = 72: %d of %d descents expand a list over 64 links, %d take a neighbour past position 64" % (through, len(q), late))
    assert through >= len(q) // 2 and late >= 5
    blob = blob.tobytes()
    ix = amd.HnswIndex(blob, 0, D)
    for k, ef in GRID:
        same(ix.search(q, k, ef), orc.hnsw_search(blob, 0, D, q, k, ef), ("m72", k, ef))


# ---- 3. the queue boundaries ----------------------------------------------------------------------------------------------------------
def boundary_sweep(amd, orc, ix, blob, metric, D, q, tag):
    """top queue: ef + 1 entries, the first hnsw_top_lds() of them in LDS -- the split and ef are moved across each other, on the
    fp32 and on the ADC traversal (the same heap code)"""
    opq, books, ocodes, rot, _, _ = opq_over_graph(amd, orc, blob, D, 16, 256)
    pairs = [(10, ef) for ef in EFS] + [(ef, ef) for ef in K_IS_EF]
    want = {p: orc.hnsw_search(blob, metric, D, q, *p) for p in pairs}
    want_adc = {p: orc.hnsw_search_adc(blob, books, ocodes, rot(q), *p) for p in pairs}
    try:
        for top_lds in TOP_LDS:
            amd.set_tuning("hnsw_top_lds", top_lds)
            for p in pairs:
                same(ix.search(q, *p), want[p], (tag, "fp32", top_lds) + p)
                same(ix.search_adc(opq, q, *p), want_adc[p], (tag, "adc", top_lds) + p)
    finally:
        amd.set_tuning("hnsw_top_lds", 256)
    return len(TOP_LDS) * len(pairs) * 2


def test_top_queue_split_tie_heavy(amd, orc):
    x = tie_heavy(6000, 16, 616)
    ix = amd.hnsw_build(x, 1, 16, 40, max_batch=1)
    boundary_sweep(amd, orc, ix, ix.save(), 1, 16, mixed_queries(x, 48, 6), "tie6000")


def test_top_queue_split_golden(amd, orc, golden):
    g = golden.hnsw
    metric, D = int(g["ip128_meta"][0]), int(g["ip128_meta"][1])
    blob = g["ip128_index"].tobytes()
    boundary_sweep(amd, orc, amd.HnswIndex(blob, metric, D), blob, metric, D, g["ip128_q"], "ip128")


def push_heap(a, v):
    """libstdc++ __push_heap on a list of (d, id), max-heap on d"""
    a.append(v)
    hole = len(a) - 1
    while hole > 0 and a[(hole - 1) // 2][0] < v[0]:
        a[hole] = a[(hole - 1) // 2]
        hole = (hole - 1) // 2
    a[hole] = v


def pop_heap(a):
    """libstdc++ __pop_heap / __adjust_heap"""
    value = a.pop()
    ln = len(a)
    if ln == 0:
        return
    hole = second = 0
    while second < (ln - 1) // 2:
        second = 2 * (second + 1)
        if a[second][0] < a[second - 1][0]:
            second -= 1
        a[hole] = a[second]
        hole = second
    if ln % 2 == 0 and second == (ln - 2) // 2:
        second = 2 * (second + 1)
        a[hole] = a[second - 1]
        hole = second - 1
    while hole > 0 and a[(hole - 1) // 2][0] < value[0]:
        a[hole] = a[(hole - 1) // 2]
        hole = (hole - 1) // 2
    a[hole] = value


def base_layer(g, dq, entry, k, ef):
    """searchBaseLayerST (hnswalg.h:217-280) over a parsed file with the query's distances dq (floats): the k results as sorted
    (distance, label) pairs, and the largest size the candidate queue reached"""
    top, cand, seen = [], [], {entry}
    push_heap(top, (dq[entry], entry))
    push_heap(cand, (-dq[entry], entry))
    lower, high = dq[entry], 1
    while cand:
        d, c = cand[0]
        if -d > lower:
            break
        pop_heap(cand)
        for nb in g["l0"][c, 1:1 + g["l0"][c, 0]].tolist():
            if nb in seen:
                continue
            seen.add(nb)
            if top[0][0] > dq[nb] or len(top) < ef:
                push_heap(cand, (-dq[nb], nb))
                push_heap(top, (dq[nb], nb))
                if len(top) > ef:
                    pop_heap(top)
                lower = top[0][0]
                high = max(high, len(cand))
    while len(top) > k:
        pop_heap(top)
    return sorted((d, int(g["labels"][i])) for d, i in top), high


def test_candidate_queue_past_its_lds_part(amd, orc):
    """ef = 1024 over 20 000 tie-heavy rows, M = 32: while the top queue fills, every unvisited neighbour (up to 64 per expanded
    node) enters the candidate queue and one leaves per expansion, so it passes HN_LCAP = 256 entries within the first dozen
    expansions.  Counted, not assumed: the level-0 loop is restated above on the parsed file, gives the oracle's answer for the
    query, and reports the queue's high-water mark -- on the fp32 distances and on the ADC distances."""
    n, D = 20000, 16
    x = tie_heavy(n, D, 2020)
    ix = amd.hnsw_build(x, 1, 32, 64, max_batch=0)
    blob = ix.save()
    g = parse(np.frombuffer(blob, np.uint8))
    q = mixed_queries(x, 32, 20)
    opq, books, ocodes, rot, _, _ = opq_over_graph(amd, orc, blob, D, 16, 256)
    want = {p: orc.hnsw_search(blob, 1, D, q, *p) for p in ((10, 1024), (1024, 1024), (10, 300))}
    want_adc = {p: orc.hnsw_search_adc(blob, books, ocodes, rot(q), *p) for p in want}
    for qi in (0, 17, 31):
        for name, dq, w in (("fp32", [float(orc.dist(1, 4, q[qi], x[i])) for i in range(n)], want[(10, 1024)]),
                            ("adc", orc.adc_scan(orc.lut(rot(q[qi:qi + 1])[0], None, books), ocodes).tolist(), want_adc[(10, 1024)])):
            res, high = base_layer(g, dq, upper_walk(g, dq)[0], 10, 1024)
            print("candidate queue, query %d, %s distances: high-water mark %d entries" % (qi, name, high))
            assert [l for _, l in res] == w[1][qi].tolist() and np.array_equal(bits([d for d, _ in res]), bits(w[0][qi]))
            assert high > 256, (qi, name, high)
    for p in want:
        same(ix.search(q, *p), want[p], ("cand", "fp32") + p)
        same(ix.search_adc(opq, q, *p), want_adc[p], ("cand", "adc") + p)


# ---- 4. many queries per slot ---------------------------------------------------------------------------------------------------------
def test_one_slot_serves_many_queries(amd, orc):
    """hnsw_slots = 1: one wave per CU, so each wave draws some twenty of the 5000 queries in turn, re-zeroing its visited bitmap
    and restarting both queues between them; a NaN query (every comparison false) and far-away queries (long descents) sit in the
    middle of the batch.  A second call with another (k, ef) follows on the same handle and scratch."""
    x = tie_heavy(6000, 16, 616)
    ix = amd.hnsw_build(x, 1, 16, 40, max_batch=1)
    blob = ix.save()
    rng = np.random.default_rng(4)
    q = mixed_queries(x, 5000, 44)
    q[1000:1500] = rng.normal(size=(500, 16)).astype(np.float32) * 50          # far from every row
    q[2000:2031] = odd_queries(x, 12)
    opq, books, ocodes, rot, _, _ = opq_over_graph(amd, orc, blob, 16, 16, 256)
    for k, ef in ((10, 50), (3, 17)):
        want, want_adc = orc.hnsw_search(blob, 1, 16, q, k, ef), orc.hnsw_search_adc(blob, books, ocodes, rot(q), k, ef)
        dflt, dflt_adc = ix.search(q, k, ef), ix.search_adc(opq, q, k, ef)
        amd.set_tuning("hnsw_slots", 1)
        try:
            one, one_adc = ix.search(q, k, ef), ix.search_adc(opq, q, k, ef)
        finally:
            amd.set_tuning("hnsw_slots", 0)
        same(one, want, ("slots=1", k, ef)); same(one, dflt, ("slots=1 against default", k, ef))
        same(one_adc, want_adc, ("slots=1 adc", k, ef)); same(one_adc, dflt_adc, ("slots=1 adc against default", k, ef))


# ---- 5. labels and ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,D", [(0, 10), (0, 16), (1, 12), (1, 7)])
def test_scattered_labels_over_duplicated_rows(amd, orc, metric, D):
    """50 groups of 8 identical rows, labels in no order (some above 2^32): which members of a group survive the cut at k is
    decided by the heaps, the order they come out in by the label.  The non-finite queries ride along: with a NaN among the
    distances the output order is what the reference's (distance, label) result queue makes of them."""
    n = 2000
    x = quarter_rows(n, D, 50 + D)
    x[100:500] = np.repeat(x[100:150], 8, axis=0)
    labels = scattered_labels(n, 5)
    ix = amd.hnsw_build(x, metric, 8, 40, labels=labels, max_batch=1)
    blob = ix.save()
    assert np.array_equal(parse(np.frombuffer(blob, np.uint8))["labels"].astype(np.int64), labels)
    q = np.ascontiguousarray(np.concatenate([x[100:500:8], odd_queries(x, 13)]))
    for k in range(1, 21):
        for ef in (k, 40):
            same(ix.search(q, k, ef), orc.hnsw_search(blob, metric, D, q, k, ef), (metric, D, k, ef))


# ---- 6. small graphs, limits, refusals --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("metric,D", [(0, 10), (1, 20)])
def test_graphs_smaller_than_k(amd, orc, metric, D, n):
    x = quarter_rows(n, D, 60 + n)
    ix = amd.hnsw_build(x, metric, 8, 40, labels=scattered_labels(n, 6), max_batch=1)     # n < M as well
    blob = ix.save()
    q = odd_queries(x, 14)
    for k, ef in ((10, 10), (10, 3), (1, 1), (3, 50)):
        d, lab = ix.search(q, k, ef)
        same((d, lab), orc.hnsw_search(blob, metric, D, q, k, ef), (metric, D, n, k, ef))
        if n < k:
            assert (lab[:, n:] == -1).all() and not bits(d[:, n:]).any()                  # padding: (+0.0f, -1), bit for bit
            assert (lab[:, :n] >= 0).all()


def test_limits_and_refusals(amd, orc):
    import torch
    x = tie_heavy(3000, 12, 312)
    ix = amd.hnsw_build(x, 1, 8, 40, max_batch=1)
    blob = ix.save()
    q = mixed_queries(x, 16, 3)
    for k, ef in ((1, 1), (20, 5), (1024, 1024), (1024, 1), (1, 1024)):
        want = orc.hnsw_search(blob, 1, 12, q, k, ef)
        same(ix.search(q, k, ef), want, ("host pointers", k, ef))
        same(ix.search(torch.from_numpy(q).cuda(), k, ef), want, ("device pointers", k, ef))
    same(ix.search(q[:1], 10, 50), orc.hnsw_search(blob, 1, 12, q[:1], 10, 50), "nq = 1")
    for k, ef in ((10, 1025), (1025, 10), (1025, 1025), (0, 10), (10, 0)):
        with pytest.raises(amd.CvtmiError):
            ix.search(q, k, ef)
    d, lab = ix.search(q[:0], 5, 10)
    assert d.shape == (0, 5) and lab.shape == (0, 5)
    d, lab = ix.search(torch.from_numpy(q[:0]).cuda(), 5, 10)
    assert tuple(d.shape) == (0, 5) and tuple(lab.shape) == (0, 5)
    same(ix.search(q, 10, 50), orc.hnsw_search(blob, 1, 12, q, 10, 50), "after the refusals")


@pytest.mark.parametrize("metric", [0, 1])
def test_default_schedule_graph_against_its_own_bytes(amd, orc, metric):
    x = tie_heavy(20000, 20, 2000 + metric)
    ix = amd.hnsw_build(x, metric, 12, 40, max_batch=0)
    blob = ix.save()
    q = mixed_queries(x, 200, 7)
    for k, ef in GRID:
        want = orc.hnsw_search(blob, metric, 20, q, k, ef)
        same(ix.search(q, k, ef), want, (metric, k, ef))
        same(amd.HnswIndex(blob, metric, 20).search(q, k, ef), want, (metric, k, ef, "reloaded"))
