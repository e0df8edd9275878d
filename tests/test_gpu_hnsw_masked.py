"""GPU: the HNSW search under a node mask (cvtmi_hnsw_search_masked and its ADC / re-rank forms, csrc/hnsw.hip: the MASKED instances).

What a result is compared with:
  * an all-ones mask: the unmasked entry of the same name on the same handle (pinned to the oracle by test_gpu_hnsw*.py), labels
    and distance bits;
  * a partial mask: `masked_base_layer` of tests/test_hnsw_masked_model.py (the level-0 rule restated on the parsed file, pinned
    on the golden graphs there) behind the unmasked greedy descent, over the oracle's own distances -- orc.dist for the fp32
    traversal, orc.adc_scan(orc.lut(...)) for the ADC one;
  * ef = k = the number of allowed nodes: the allowed nodes reachable from the level-0 entry, sorted.
Rows are quantised to quarters and partly repeated, so equal distances are common and the heaps decide."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

from conftest import bits
from test_gpu_hnsw import _graph_labels, opq_over_graph
from test_gpu_hnsw_build import parse, tie_heavy
from test_gpu_hnsw_edges import mixed_queries, pq_layouts, same, upper_walk
from test_hnsw_masked_model import masked_base_layer, padded, reachable
from test_oracle_hnsw_edges import GRID, odd_queries, quarter_rows, scattered_labels

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
SHAPES = [(0, 10), (0, 20), (1, 7), (1, 20), (1, 16)]     # every DistF32 instance: <IP,1> <IP,4> <L2,1> <L2,4> <L2,8>
NQ = 48
EINVAL, EUNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()
    return cvt_amd


def words_of(allowed, extra=0, garbage=False):
    """uint64 words of a bool array: bit i & 63 of word i >> 6 = node i.  extra: all-ones words appended behind ceil(n / 64);
    garbage: the bits of the last word at positions >= n are set"""
    n = allowed.shape[0]
    padded_bits = np.zeros((n + 63) // 64 * 64, bool)
    padded_bits[:n] = allowed
    if garbage:
        padded_bits[n:] = True
    w = np.packbits(padded_bits, bitorder="little").view("<u8").astype(np.uint64)
    return np.ascontiguousarray(np.concatenate([w, np.full(extra, ~np.uint64(0), np.uint64)]))


class Graph:
    """a built graph with its parsed file, queries, and the oracle's distance of every query to every node (made on first use)"""
    def __init__(self, amd, orc, metric, D, x, labels=None, M=8, efc=40, nq=NQ):
        self.metric, self.D, self.x, self.orc = metric, D, x, orc
        self.ix = amd.hnsw_build(x, metric, M, efc, labels=labels, max_batch=1)
        self.blob = self.ix.save()
        self.g = parse(self.blob)
        self.n = x.shape[0]
        self.q = mixed_queries(x, nq, 100 + D + metric)
        self._dq = {}

    def dq(self, qi):
        if qi not in self._dq:
            self._dq[qi] = [self.orc.dist(self.metric, 4, self.q[qi], self.x[i]) for i in range(self.n)]
        return self._dq[qi]


def model(g, dqs, k, ef, allowed):
    """the masked search of every query whose distances dqs lists: (distances [nq][k], labels [nq][k], candidate high-water marks)"""
    out_d, out_l, highs = [], [], []
    for dq in dqs:
        res, high = masked_base_layer(g, dq, upper_walk(g, dq)[0], k, ef, allowed)
        d, lab = padded(res, k)
        out_d.append(d); out_l.append(lab); highs.append(high)
    return np.stack(out_d), np.stack(out_l), highs


@pytest.fixture(scope="module")
def built(amd, orc):
    cache = {}

    def get(metric, D):
        if (metric, D) not in cache:
            cache[(metric, D)] = Graph(amd, orc, metric, D, tie_heavy(2000, D, 300 + D + metric))
        return cache[(metric, D)]
    return get


# ---- 1. all-ones == unmasked ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,D", SHAPES)
def test_all_ones_mask_is_the_unmasked_search(amd, orc, built, metric, D):
    """fp32 over GRID, ADC on every PQ layout of the width (M = 16 and M = 8 / 4 at D = 16, M = 4 at D = 20) and the re-rank chain;
    non-finite queries ride along; all-ones words behind the mask and garbage bits past n change nothing"""
    import torch
    G = built(metric, D)
    ix, n = G.ix, G.n
    q = np.ascontiguousarray(np.concatenate([G.q, odd_queries(G.x, 7 + D)]))
    ones = np.ones(n, bool)
    forms = {"bool": ones, "words": words_of(ones), "extra": words_of(ones, extra=3), "garbage": words_of(ones, garbage=True)}
    for k, ef in GRID:
        want = ix.search(q, k, ef)
        for name, m in forms.items():
            same(ix.search_masked(q, k, ef, m), want, (metric, D, k, ef, name))
    qd = torch.from_numpy(q).cuda()
    md = torch.from_numpy(words_of(ones, extra=1, garbage=True).view(np.int64)).cuda()
    same(ix.search_masked(qd, 10, 50, md), ix.search(q, 10, 50), (metric, D, "device pointers"))
    same(ix.search_masked(qd, 10, 50, torch.from_numpy(ones).cuda()), ix.search(q, 10, 50), (metric, D, "device bool"))
    for M, K in pq_layouts(D)[:2]:
        opq, _, _, _, _, _ = opq_over_graph(amd, orc, G.blob, D, M, K)
        for k, ef in ((10, 50), (100, 300), (1, 1)):
            same(ix.search_adc_masked(opq, q, k, ef, forms["garbage"]), ix.search_adc(opq, q, k, ef), (metric, D, M, k, ef, "adc"))
        same(ix.search_adc_masked(opq, qd, 10, 50, md), ix.search_adc(opq, q, 10, 50), (metric, D, M, "adc device pointers"))
        for k, ef, rr in ((5, 40, 40), (10, 64, 30), (1, 16, 8)):
            same(ix.search_adc_rerank_masked(opq, q, k, ef, forms["extra"], rr), ix.search_adc_rerank(opq, q, k, ef, rr), (metric, D, M, k, ef, rr))
        same(ix.search_adc_rerank_masked(opq, qd, 5, 40, md, 40), ix.search_adc_rerank(opq, q, 5, 40, 40), (metric, D, M, "rerank device"))
        opq.close()


@pytest.mark.parametrize("case", ["ip32", "l2f16", "ip20", "l2f7", "ip128"])
def test_all_ones_mask_on_golden_graphs(amd, orc, golden, case):
    z = golden.hnsw
    metric, D, n = (int(v) for v in z[case + "_meta"][:3])
    blob = z[case + "_index"].tobytes()
    ix = amd.HnswIndex(blob, metric, D)
    q = z[case + "_q"]
    ones = words_of(np.ones(n, bool), extra=2, garbage=True)
    for k, ef in GRID:
        same(ix.search_masked(q, k, ef, ones), ix.search(q, k, ef), (case, k, ef))
    if case == "ip128":
        opq, _, _, _, _, _ = opq_over_graph(amd, orc, blob, D, 16, 256)
        same(ix.search_adc_masked(opq, q, 10, 64, ones), ix.search_adc(opq, q, 10, 64), (case, "adc"))
        same(ix.search_adc_rerank_masked(opq, q, 5, 64, ones, 32), ix.search_adc_rerank(opq, q, 5, 64, 32), (case, "rerank"))
        opq.close()
    ix.close()


@pytest.mark.parametrize("n", [1, 5])
def test_all_ones_mask_pads_on_graphs_smaller_than_k(amd, n):
    x = quarter_rows(n, 12, 60 + n)
    ix = amd.hnsw_build(x, 1, 8, 40, labels=scattered_labels(n, 6), max_batch=1)
    q = odd_queries(x, 14)
    d, lab = ix.search_masked(q, 10, 10, np.ones(n, bool))
    same((d, lab), ix.search(q, 10, 10), n)
    assert (lab[:, n:] == -1).all() and not bits(d[:, n:]).any() and (lab[:, :n] >= 0).all()      # padding: (+0.0f, -1)
    d, lab = ix.search_masked(q, 10, 3, np.zeros(n, bool))
    assert (lab == -1).all() and not bits(d).any()
    ix.close()


# ---- 2. partial masks == model ----------------------------------------------------------------------------------------------------------
def partial_masks(G, seed):
    n = G.n
    rng = np.random.default_rng(seed)
    entries = sorted({upper_walk(G.g, G.dq(qi))[0] for qi in range(G.q.shape[0])} | {int(G.g["ep"])})
    masks = {"d0.5": rng.random(n) < 0.5, "d0.1": rng.random(n) < 0.1, "d0.02": rng.random(n) < 0.02}
    masks["alternate words"] = (np.arange(n) // 64) % 2 == 0
    one = np.zeros(n, bool); one[int(rng.integers(0, n))] = True
    masks["one node"] = one
    with_e = masks["d0.1"].copy(); with_e[entries] = True
    without_e = masks["d0.5"].copy(); without_e[entries] = False
    masks["entries allowed"], masks["entries disallowed"] = with_e, without_e
    masks["none"] = np.zeros(n, bool)
    return masks


@pytest.mark.parametrize("metric,D", SHAPES)
def test_partial_masks_match_the_model(amd, orc, built, metric, D):
    G = built(metric, D)
    dqs = [G.dq(qi) for qi in range(NQ)]
    for name, allowed in partial_masks(G, 11 * D + metric).items():
        w = words_of(allowed, garbage=True)
        for k, ef in GRID:
            d, lab = G.ix.search_masked(G.q, k, ef, w)
            if name == "none":                                             # nothing may be a result: everything pads
                assert (lab == -1).all() and not bits(d).any(), (metric, D, k, ef)
                continue
            wd, wl, _ = model(G.g, dqs, k, ef, allowed)
            assert np.array_equal(lab, wl), (metric, D, name, k, ef)
            assert np.array_equal(bits(d), bits(wd)), (metric, D, name, k, ef)
            assert (lab < 0).all() or allowed[np.isin(G.g["labels"].astype(np.int64), lab[lab >= 0])].all()


@pytest.mark.parametrize("M,K", [(16, 256), (8, 64)])
def test_partial_masks_match_the_model_over_codes(amd, orc, built, M, K):
    """ADC and ADC + re-rank at D = 16: the same rule over the oracle's ADC distances; the re-rank sees the masked list alone"""
    G = built(1, 16)
    opq, books, ocodes, rot, xv, _ = opq_over_graph(amd, orc, G.blob, 16, M, K)
    nq = 24
    q = G.q[:nq]
    qr = rot(q)
    dqs = [orc.adc_scan(orc.lut(qr[qi], None, books), ocodes).tolist() for qi in range(nq)]
    masks = partial_masks(G, 5 + M)
    lab2row = {int(l): r for r, l in enumerate(_graph_labels(G.blob, 16))}
    for name in ("d0.5", "d0.02", "alternate words", "entries disallowed"):
        allowed = masks[name]
        w = words_of(allowed)
        for k, ef in ((10, 10), (10, 50), (100, 300)):
            d, lab = G.ix.search_adc_masked(opq, q, k, ef, w)
            wd, wl, _ = model(G.g, dqs, k, ef, allowed)
            assert np.array_equal(lab, wl) and np.array_equal(bits(d), bits(wd)), (M, name, k, ef)
        for k, ef, rr in ((5, 40, 40), (10, 64, 30)):
            d, lab = G.ix.search_adc_rerank_masked(opq, q, k, ef, w, rr)
            _, cand, _ = model(G.g, dqs, rr, ef, allowed)                  # labels of the masked ADC list, ADC order
            for qi in range(nq):
                rows = [lab2row[int(l)] for l in cand[qi] if l >= 0]
                ex = np.array([orc.dist(1, 4, q[qi], xv[r]) for r in rows], dtype=np.float32)
                order = np.argsort(ex, kind="stable")[:k]
                want_l = [int(cand[qi][j]) for j in order]
                assert lab[qi, :len(want_l)].tolist() == want_l and (lab[qi, len(want_l):] == -1).all(), (M, name, k, ef, rr, qi)
                assert np.array_equal(bits(d[qi, :len(want_l)]), bits(ex[order])), (M, name, k, ef, rr, qi)
    opq.close()


@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_tail_word_of_small_graphs(amd, orc, n):
    """the last mask word at 63, 64 (exactly one word), 65 and 130 (two and a bit) nodes, with garbage behind node n - 1"""
    G = Graph(amd, orc, 1, 12, quarter_rows(n, 12, 70 + n, dup=20), nq=16)
    dqs = [G.dq(qi) for qi in range(16)]
    rng = np.random.default_rng(n)
    last = np.zeros(n, bool); last[n - 1] = True
    for name, allowed in (("half", rng.random(n) < 0.5), ("last node", last), ("all but the last", ~last), ("last word", np.arange(n) >= (n - 1) // 64 * 64)):
        for k, ef in ((1, 1), (10, 10), (100, 300)):
            wd, wl, _ = model(G.g, dqs, k, ef, allowed)
            for w in (words_of(allowed), words_of(allowed, extra=2, garbage=True)):
                d, lab = G.ix.search_masked(G.q, k, ef, w)
                assert np.array_equal(lab, wl) and np.array_equal(bits(d), bits(wd)), (n, name, k, ef)
    G.ix.close()


# ---- 3. the exhaustive property ---------------------------------------------------------------------------------------------------------
def check_exhaustive(ix, g, q, dqs, allowed, tag):
    cnt = int(allowed.sum())
    assert 1 <= cnt <= 1000
    d, lab = ix.search_masked(q, cnt, cnt, words_of(allowed))
    reach = {}
    for qi, dq in enumerate(dqs):
        entry = upper_walk(g, dq)[0]
        if entry not in reach:
            reach[entry] = reachable(g, entry)
        want = sorted((dq[i], int(g["labels"][i])) for i in np.flatnonzero(allowed).tolist() if i in reach[entry])
        wd, wl = padded(want, cnt)
        assert np.array_equal(lab[qi], wl) and np.array_equal(bits(d[qi]), bits(wd)), (tag, cnt, qi)
    return min(len(r) for r in reach.values())


def test_exhaustive_walk_returns_the_allowed_reachable_set(amd, orc, built, golden):
    """ef = k = the number of allowed nodes: the walk ends on an empty candidate queue only, and the answer is exactly the allowed
    nodes the level-0 links reach from the entry, in ascending (distance, label) -- on a built graph and on the l2f16 golden, where
    the entry does not reach every node"""
    G = built(1, 16)
    rng = np.random.default_rng(3)
    one = np.zeros(G.n, bool); one[G.n // 3] = True
    for allowed in (rng.random(G.n) < 0.3, rng.random(G.n) < 0.05, one):
        check_exhaustive(G.ix, G.g, G.q, [G.dq(qi) for qi in range(NQ)], allowed, "built")
    z = golden.hnsw
    metric, D, n = (int(v) for v in z["l2f16_meta"][:3])
    blob = z["l2f16_index"].tobytes()
    g = parse(blob)
    q = np.ascontiguousarray(z["l2f16_q"][:16], np.float32)
    dqs = [[orc.dist(metric, 4, q[qi], g["rows"][i]) for i in range(n)] for qi in range(q.shape[0])]
    ix = amd.HnswIndex(blob, metric, D)
    fewest = min(check_exhaustive(ix, g, q, dqs, allowed, "l2f16") for allowed in (rng.random(n) < 0.4, rng.random(n) < 0.02))
    assert fewest < n, "the l2f16 golden has nodes its level-0 entry does not reach"
    ix.close()


# ---- 4. the candidate queue past the unmasked bound --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["l2f16", "ip32"])
def test_candidate_queue_past_the_unmasked_bound(amd, orc, golden, case):
    """(k, ef) = (10, 16) under sparse masks: while fewer than ef allowed nodes have been found nothing is pruned and every visited
    node is queued.  Counted on the model: the queue's high-water mark is above the unmasked plan's 2 ef maxM0 entries and above
    the 256 entries held in LDS, and within the capacity the masked plan reserves (n entries: cvtmi_hnsw_last_masked)."""
    z = golden.hnsw
    metric, D, n = (int(v) for v in z[case + "_meta"][:3])
    blob = z[case + "_index"].tobytes()
    g = parse(blob)
    q = np.ascontiguousarray(z[case + "_q"][:16], np.float32)
    dqs = [[orc.dist(metric, 4, q[qi], g["rows"][i]) for i in range(n)] for qi in range(q.shape[0])]
    ix = amd.HnswIndex(blob, metric, D)
    rng = np.random.default_rng(len(case))
    for dens in (0.02, 0.01):
        allowed = rng.random(n) < dens
        wd, wl, highs = model(g, dqs, 10, 16, allowed)
        bound = 2 * 16 * g["maxM0"]
        over = sum(h > bound for h in highs)
        print("%s density %.2f: candidate high-water marks %d .. %d, %d of %d queries above 2 ef maxM0 = %d" % (case, dens, min(highs), max(highs), over, len(highs), bound))
        # every query's queue leaves LDS, and most pass what the unmasked plan would have reserved (measured on the model, CPU:
        # l2f16 399 .. 710 and 930 .. 997 against 384; ip32 501 .. 890 and 1219 .. 1533 against 512)
        assert min(highs) > 256 and over >= len(highs) // 2, (case, dens, highs)
        d, lab = ix.search_masked(q, 10, 16, words_of(allowed))
        slots, cap, scratch, form = ix.last_masked()
        assert max(highs) <= cap and cap >= n and slots >= 1 and scratch > 0 and form == 0, (slots, cap, scratch, form)
        assert np.array_equal(lab, wl) and np.array_equal(bits(d), bits(wd)), (case, dens)
    ix.close()


# ---- 5. queue splits and slots -------------------------------------------------------------------------------------------------------------
def test_queue_splits_slots_and_tables_change_nothing(amd, orc, built):
    G = built(1, 16)
    rng = np.random.default_rng(55)
    allowed = rng.random(G.n) < 0.1
    w = words_of(allowed)
    q = mixed_queries(G.x, 300, 56)
    q[:NQ] = G.q
    want = {p: G.ix.search_masked(q, *p, w) for p in ((10, 50), (100, 300))}
    wd, wl, _ = model(G.g, [G.dq(qi) for qi in range(8)], 10, 50, allowed)
    assert np.array_equal(want[(10, 50)][1][:8], wl) and np.array_equal(bits(want[(10, 50)][0][:8]), bits(wd))
    slots_default = G.ix.last_masked()[0]
    amd.set_tuning("hnsw_slots", 1)                                        # one wave per CU: bitmap and queues are reused between queries
    try:
        for p in want:
            same(G.ix.search_masked(q, *p, w), want[p], ("slots=1",) + p)
        assert 1 <= G.ix.last_masked()[0] <= slots_default
    finally:
        amd.set_tuning("hnsw_slots", 0)
    for top_lds in (0, 17, 256):
        amd.set_tuning("hnsw_top_lds", top_lds)
        try:
            for p in want:
                same(G.ix.search_masked(q, *p, w), want[p], ("top_lds", top_lds) + p)
        finally:
            amd.set_tuning("hnsw_top_lds", 256)
    opq, _, _, _, _, _ = opq_over_graph(amd, orc, G.blob, 16, 16, 256)
    got = {}
    for tables_in_lds in (0, 1):
        amd.set_tuning("hnsw_adc_tables", tables_in_lds)
        try:
            got[tables_in_lds] = (G.ix.search_adc_masked(opq, q, 10, 50, w), G.ix.search_adc_rerank_masked(opq, q, 5, 40, w, 40))
            assert G.ix.last_masked()[3] == 1 + tables_in_lds
        finally:
            amd.set_tuning("hnsw_adc_tables", 0)
    same(got[1][0], got[0][0], "adc tables in LDS"); same(got[1][1], got[0][1], "rerank tables in LDS")
    opq.close()


# ---- 6. mask_from_labels ---------------------------------------------------------------------------------------------------------------------
def test_mask_from_labels(amd, orc):
    import torch
    n, D = 2000, 10
    x = quarter_rows(n, D, 91)
    labels = scattered_labels(n, 9)
    ix = amd.hnsw_build(x, 0, 8, 40, labels=labels, max_batch=1)
    stored = parse(ix.save())["labels"].astype(np.int64)
    assert np.array_equal(stored, labels)
    rng = np.random.default_rng(10)
    picked = labels[rng.random(n) < 0.2]
    foreign = np.array([-1, 1 << 62, (1 << 40) + 7, 3 << 20], np.int64)
    foreign = foreign[~np.isin(foreign, labels)]
    sets = {"picked": picked, "shuffled with duplicates and foreign": rng.permutation(np.concatenate([picked, picked[:50], foreign])),
            "empty": np.zeros(0, np.int64), "all": labels[::-1].copy(), "one": labels[n - 1:]}
    for name, s in sets.items():
        want = np.isin(stored, s)
        for words in (None, (n + 63) // 64 + 3):
            m = ix.mask_from_labels(s, words)
            assert m.dtype == np.uint64 and m.shape[0] == ((n + 63) // 64 if words is None else words), name
            assert np.array_equal(m, np.concatenate([words_of(want), np.zeros(m.shape[0] - (n + 63) // 64, np.uint64)])), name   # bits past n: cleared
        if s.shape[0]:
            md = ix.mask_from_labels(torch.from_numpy(s).cuda(), (n + 63) // 64 + 1)
            assert np.array_equal(md.cpu().numpy().view(np.uint64)[:-1], words_of(want)) and int(md[-1]) == 0, name
    q = mixed_queries(x, 16, 92)
    m = ix.mask_from_labels(picked)
    d, lab = ix.search_masked(q, 10, 50, m)
    assert np.isin(lab, picked).all()
    same(ix.search_masked(q, 10, 50, np.isin(stored, picked)), (d, lab), "bool mask against the label mask")
    ix.close()


# ---- 7. argument checks and concurrency ----------------------------------------------------------------------------------------------------
def test_argument_checks_leave_the_handle_usable(amd, orc, built):
    G = built(1, 16)
    lib = amd.lib()
    h = G.ix.h
    nq, k = 4, 10
    q = np.ascontiguousarray(G.q[:nq])
    d = np.empty((nq, k), np.float32); lab = np.empty((nq, k), np.int64)
    ones = words_of(np.ones(G.n, bool))
    p = lambda a: C.c_void_p(a.ctypes.data)
    null = C.c_void_p(0)
    call = lambda qq, n_, k_, ef_, m_, mw_, d_, l_: lib.cvtmi_hnsw_search_masked(h, qq, C.c_int64(n_), C.c_int(k_), C.c_int(ef_), m_, C.c_int64(mw_), d_, l_)
    full = ones.shape[0]
    assert call(p(q), nq, k, 50, p(ones), full - 1, p(d), p(lab)) == EINVAL and b"mask words" in lib.cvtmi_last_error()     # short mask
    assert call(p(q), nq, k, 50, null, full, p(d), p(lab)) == EINVAL                                                          # NULL mask
    assert call(null, nq, k, 50, p(ones), full, p(d), p(lab)) == EINVAL
    assert call(p(q), nq, k, 50, p(ones), full, null, p(lab)) == EINVAL
    assert call(p(q), nq, k, 50, p(ones), full, p(d), null) == EINVAL
    assert call(p(q), -1, k, 50, p(ones), full, p(d), p(lab)) == EINVAL
    assert call(p(q), nq, k, 50, p(ones), -1, p(d), p(lab)) == EINVAL
    for kk, ef in ((10, 1025), (1025, 10), (0, 10), (10, 0)):                                                                 # as the unmasked entry answers
        assert call(p(q), nq, kk, ef, p(ones), full, p(d), p(lab)) == EUNSUPPORTED, (kk, ef)
        with pytest.raises(amd.CvtmiError):
            G.ix.search(q, kk, ef)
    assert call(null, 0, k, 50, null, full, null, null) == 0                                                                  # nq == 0 does nothing
    with pytest.raises(amd.CvtmiError):
        G.ix.search_masked(q, 10, 50, ones[:-1])
    with pytest.raises(amd.CvtmiError):
        G.ix.mask_from_labels(np.arange(5, dtype=np.int64), full - 1)
    opq, _, _, _, _, _ = opq_over_graph(amd, orc, G.blob, 16, 16, 256)
    with pytest.raises(amd.CvtmiError):
        G.ix.search_adc_masked(opq, q, 10, 50, ones[:-1])
    with pytest.raises(amd.CvtmiError):
        G.ix.search_adc_rerank_masked(opq, q, 10, 40, ones, 5)            # rerank < k is refused, as unmasked
    with pytest.raises(amd.CvtmiError):
        G.ix.search_adc_masked(opq, q, 10, 1025, ones)
    opq.close()
    assert call(p(q), nq, k, 50, p(ones), full, p(d), p(lab)) == 0
    same((d, lab), G.ix.search(q, k, 50), "after the refusals")


def test_concurrent_masked_and_unmasked_searches(amd, orc, built):
    """four host threads on one handle, masked and unmasked, each on a leased scratch set with its own staged mask: every call
    returns what it returns alone"""
    G = built(1, 16)
    rng = np.random.default_rng(77)
    m1, m2 = words_of(rng.random(G.n) < 0.1), words_of(rng.random(G.n) < 0.5)
    jobs = [("masked 10%", lambda: G.ix.search_masked(G.q, 10, 50, m1)), ("unmasked", lambda: G.ix.search(G.q, 10, 50)),
            ("masked 50%", lambda: G.ix.search_masked(G.q, 20, 20, m2)), ("unmasked small", lambda: G.ix.search(G.q[:5], 3, 16))]
    want = {name: fn() for name, fn in jobs}
    bad, start = [], threading.Barrier(len(jobs))

    def worker(name, fn):
        start.wait()
        for _ in range(10):
            d, l = fn()
            if not (np.array_equal(l, want[name][1]) and np.array_equal(bits(d), bits(want[name][0]))):
                bad.append(name)
                return
    ts = [threading.Thread(target=worker, args=j) for j in jobs]
    for t in ts: t.start()
    for t in ts: t.join()
    assert not bad, bad


# ---- 8. host mirror and CLI ------------------------------------------------------------------------------------------------------------------
def test_hnsw_search_cli_allow(amd, tmp_path, golden):
    """hnsw_search --allow FILE (the mirror's searchKnnBatch with a BaseFilterFunctor) on a golden file == search_masked with
    mask_from_labels; without the option the file's own answers, as before"""
    z = golden.hnsw
    case = "l2f16"
    metric, D, n, M, efc, k, ef = (int(v) for v in z[case + "_meta"])
    blob = z[case + "_index"].tobytes()
    q = np.ascontiguousarray(z[case + "_q"], np.float32)
    (tmp_path / "g.hnsw").write_bytes(blob)
    (tmp_path / "q.bin").write_bytes(q.tobytes())
    labels = parse(blob)["labels"].astype(np.int64)
    rng = np.random.default_rng(8)
    allow = np.concatenate([labels[rng.random(n) < 0.05], [int(labels.max()) + 5]])      # a foreign label is fine
    (tmp_path / "allow.txt").write_text("".join("%d\n" % v for v in allow))
    r = subprocess.run([os.path.join(BIN, "hnsw_search"), "g.hnsw", "q.bin", str(D), str(k), str(ef), "out.txt", "l2", "--allow", "allow.txt"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ix = amd.HnswIndex(blob, metric, D)
    d, lab = ix.search_masked(q, k, ef, ix.mask_from_labels(allow))
    lines = (tmp_path / "out.txt").read_text().splitlines()
    assert len(lines) == q.shape[0]
    for qi, line in enumerate(lines):
        pairs = [t.split(":") for t in line.split()]
        m = len(pairs)
        assert [int(t[0]) for t in pairs] == lab[qi, :m].tolist() and (lab[qi, m:] == -1).all(), qi
        assert np.array_equal(bits(np.array([float(t[1]) for t in pairs], np.float32)), bits(d[qi, :m])), qi
    assert np.isin(lab[lab >= 0], allow).all()
    ix.close()
