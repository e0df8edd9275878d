"""CPU: the level-0 rule of the masked HNSW search (cvtmi_hnsw_search_masked) restated in Python on parsed graph
files, and pinned on the five golden graphs.

The rule is current hnswlib's searchBaseLayerST with isIdAllowed: the mask decides what may enter the RESULT queue and never what
is traversed, and the walk may only stop on a full result queue.  Two properties tie it to things that are specified elsewhere:
  * under an all-ones mask it returns what the unmasked search returns -- the oracle's orc.hnsw_search, labels and distance bits;
  * with ef >= the number of allowed nodes it returns exactly the allowed nodes that can be reached from the level-0 entry node
    over level-0 links, in ascending (distance, label).
tests/test_gpu_hnsw_masked.py compares the kernel with `masked_base_layer` on partial masks."""
import numpy as np
import pytest

from conftest import bits
from test_gpu_hnsw_build import parse
from test_gpu_hnsw_edges import pop_heap, push_heap, upper_walk
from test_oracle_hnsw_edges import GRID

CASES = ("ip32", "l2f16", "ip20", "l2f7", "ip128")
NQ = 8


def neighbours(g):
    """the level-0 lists of a parsed file as Python lists, in list order (made once per graph)"""
    if "nbrs" not in g:
        g["nbrs"] = [row[1:1 + row[0]].tolist() for row in g["l0"]]
    return g["nbrs"]


def masked_base_layer(g, dq, entry, k, ef, allowed):
    """Level 0 of the masked search over a parsed file: dq = the query's distance to every node (floats), allowed = one bool per
    node.  Returns the results as (distance, label) pairs in ascending order (fewer than k: the caller pads) and the largest size
    the candidate queue reached."""
    efe = max(ef, k)
    nbrs = neighbours(g)
    top, cand, seen = [], [], {entry}
    lower = float("inf")
    if allowed[entry]:
        push_heap(top, (dq[entry], entry))
        lower = dq[entry]
    push_heap(cand, (-dq[entry], entry))
    high = 1
    while cand:
        d, c = cand[0]
        if -d > lower and len(top) >= efe:          # with a filter the walk may only stop on a FULL result queue
            break
        pop_heap(cand)
        for nb in nbrs[c]:
            if nb in seen:
                continue
            seen.add(nb)
            if len(top) < efe or lower > dq[nb]:
                push_heap(cand, (-dq[nb], nb))       # traversed whether allowed or not
                if allowed[nb]:
                    push_heap(top, (dq[nb], nb))
                    if len(top) > efe:
                        pop_heap(top)
                if top:
                    lower = top[0][0]
                high = max(high, len(cand))
    while len(top) > k:
        pop_heap(top)
    return sorted((d, int(g["labels"][i])) for d, i in top), high


def padded(res, k):
    """(distances [k] float32, labels [k] int64) of a result list, padded as cvtmi_hnsw_search pads: (+0.0f, -1)"""
    d = np.zeros(k, np.float32)
    lab = np.full(k, -1, np.int64)
    d[:len(res)] = [r[0] for r in res]
    lab[:len(res)] = [r[1] for r in res]
    return d, lab


def reachable(g, entry):
    """nodes the level-0 links lead to from `entry` (the entry included)"""
    nbrs = neighbours(g)
    seen, todo = {entry}, [entry]
    while todo:
        c = todo.pop()
        for nb in nbrs[c]:
            if nb not in seen:
                seen.add(nb)
                todo.append(nb)
    return seen


def query_distances(orc, metric, rows, q):
    """the oracle's distance of one query to every row, as Python floats"""
    return [orc.dist(metric, 4, q, rows[i]) for i in range(rows.shape[0])]


@pytest.fixture(scope="module")
def graphs(orc, golden):
    out = {}
    for case in CASES:
        z = golden.hnsw
        metric, D = int(z[case + "_meta"][0]), int(z[case + "_meta"][1])
        blob = z[case + "_index"].tobytes()
        g = parse(blob)
        q = np.ascontiguousarray(z[case + "_q"][:NQ], np.float32)
        dq = [query_distances(orc, metric, g["rows"], q[i]) for i in range(q.shape[0])]
        out[case] = (metric, D, blob, g, q, dq)
    return out


@pytest.mark.parametrize("case", CASES)
def test_all_ones_mask_is_the_unmasked_search(orc, graphs, case):
    """While the result queue is not full every candidate is also in it, so `-c.d > lower` cannot hold and the extra stop condition
    is vacuous: the same walk, the same heaps, the same answer as searchKnn."""
    metric, D, blob, g, q, dq = graphs[case]
    ones = np.ones(g["cnt"], bool)
    for k, ef in GRID:
        od, ol = orc.hnsw_search(blob, metric, D, q, k, ef)
        for qi in range(q.shape[0]):
            res, _ = masked_base_layer(g, dq[qi], upper_walk(g, dq[qi])[0], k, ef, ones)
            d, lab = padded(res, k)
            assert np.array_equal(lab, ol[qi]), (case, k, ef, qi)
            assert np.array_equal(bits(d), bits(od[qi])), (case, k, ef, qi)


@pytest.mark.parametrize("case", CASES)
def test_exhaustive_walk_returns_the_allowed_reachable_set(orc, graphs, case):
    """ef = k = the number of allowed nodes: the result queue can fill at best with the last allowed node, so the walk ends on an
    empty candidate queue and every reachable node has been expanded.  Two goldens are not fully reachable from the entry node
    (l2f16, l2f7): the set really is the reachable one."""
    metric, D, blob, g, q, dq = graphs[case]
    n = g["cnt"]
    rng = np.random.default_rng(len(case) + n)
    masks = [rng.random(n) < dens for dens in (0.3, 0.05, 0.01)]
    one = np.zeros(n, bool); one[n // 3] = True
    masks.append(one)
    unreached = 0
    for allowed in masks:
        cnt = int(allowed.sum())
        assert 1 <= cnt <= 1000
        for qi in range(q.shape[0]):
            entry = upper_walk(g, dq[qi])[0]
            reach = reachable(g, entry)
            unreached += len(reach) < n
            want = sorted((dq[qi][i], int(g["labels"][i])) for i in np.flatnonzero(allowed).tolist() if i in reach)
            res, high = masked_base_layer(g, dq[qi], entry, cnt, cnt, allowed)
            assert res == want, (case, cnt, qi)
            assert high <= n
    if case in ("l2f16", "l2f7"):
        assert unreached > 0, "these two graphs have nodes the level-0 entry does not reach"
