"""GPU: deleted nodes of an HNSW graph (cvtmi_hnsw_mark_deleted and its companions).

Everything is compared bit for bit:
  * a search on a handle with dead set S == the `_masked` entry of the same name on an untouched twin of the graph under "not S"
    (the caller's mask m: under m & ~S) -- fp32 on every DistF32 instance, ADC on M = 16 / 8 / 4, the re-rank chain, device pointers,
    tail words at 63 / 64 / 65 / 130 nodes with garbage in the caller's tail bits, all nodes dead;
  * the state (changed, deleted_count, deleted_mask) == np.isin over the graph's labels; unmarking everything puts the handle back
    on the unmasked kernels (launch log);
  * files: the mark is bit 16 of the count word and nothing else changes, load reproduces state and answers, bit 17 is refused, the
    host CLI's marked file is the handle's;
  * cvtmi_hnsw_add on a marked graph: max_batch = 1 writes the host mirror's file (hnsw_delete + hnsw_add, pinned to the model on the
    CPU by tests/test_host_hnsw_delete.py), batches of 2, 7 and the default schedule write the file of tests/hnsw_delete_model.py --
    for the dead sets "entry point alone / a random third / all but one / all / none", a dead hub, a top level raised past a dead
    entry point, an add across bitmap words and a doubling of device storage, and a case whose candidate queue passes what the
    construction without deletions reserves;
  * without deletions cvtmi_hnsw_add launches the kernels it always launched."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import hnsw_build_model as hm
import hnsw_delete_model as dm
from conftest import bits
from test_gpu_hnsw import opq_over_graph
from test_gpu_hnsw_build import parse, tie_heavy
from test_gpu_hnsw_edges import mixed_queries, pq_layouts, same
from test_gpu_hnsw_masked import SHAPES, words_of
from test_host_hnsw_add import host_add
from test_host_hnsw_delete import DEAD_SETS, dead_set, extra_rows, host_delete
from test_oracle_hnsw_edges import quarter_rows, scattered_labels

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
EINVAL = -1
N, NQ = 600, 48
GRID = ((1, 1), (10, 50), (100, 300))


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()
    return cvt_amd


class Pair:
    """a graph file, its parsed form, queries, and two handles of it: `ix` (gets the marks) and `twin` (never touched)"""
    def __init__(self, amd, metric, D, x, labels=None, M=8, efc=32, nq=NQ):
        self.metric, self.D, self.n = metric, D, x.shape[0]
        self.twin = amd.hnsw_build(x, metric, M, efc, labels=labels, max_batch=1)
        self.blob = self.twin.save()
        self.g = parse(self.blob)
        self.labels = self.g["labels"].astype(np.int64)
        self.ix = amd.HnswIndex(self.blob, metric, D)
        self.q = mixed_queries(x, nq, 100 + D + metric)

    def close(self):
        self.ix.close()
        self.twin.close()


@pytest.fixture(scope="module")
def pairs(amd):
    cache = {}

    def get(metric, D):
        if (metric, D) not in cache:
            cache[(metric, D)] = Pair(amd, metric, D, tie_heavy(N, D, 300 + D + metric), labels=scattered_labels(N, D).view(np.uint64))
        return cache[(metric, D)]
    yield get
    for p in cache.values():
        p.close()


def saved(idx):
    return np.frombuffer(idx.save(), dtype=np.uint8)


def marked_only(P, S):
    """P.ix with exactly the nodes S (bool [n]) dead"""
    P.ix.unmark_deleted(P.labels)
    P.ix.mark_deleted(P.labels[S])
    assert P.ix.deleted_count() == int(S.sum())


# ---- 1. search == mask -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,D", SHAPES)
def test_fp32_search_equals_masked_twin(amd, pairs, metric, D):
    import torch
    P = pairs(metric, D)
    rng = np.random.default_rng(7 * D + metric)
    S = rng.random(P.n) < 0.33
    S[P.g["ep"]] = True
    marked_only(P, S)
    m = rng.random(P.n) < 0.5
    for k, ef in GRID:
        same(P.ix.search(P.q, k, ef), P.twin.search_masked(P.q, k, ef, words_of(~S)), (metric, D, k, ef, "unmasked entry"))
        assert P.ix.last_masked()[3] == 0 and P.ix.last_masked()[1] >= P.n          # reported as a masked search, a queue of n entries
        got = P.ix.search_masked(P.q, k, ef, words_of(m, extra=1, garbage=True))
        same(got, P.twin.search_masked(P.q, k, ef, words_of(m & ~S)), (metric, D, k, ef, "masked entry"))
    qd = torch.from_numpy(P.q).cuda()
    md = torch.from_numpy(words_of(m, garbage=True).view(np.int64)).cuda()
    keep = md.clone()
    same(P.ix.search(qd, 10, 50), P.twin.search_masked(P.q, 10, 50, words_of(~S)), (metric, D, "device"))
    same(P.ix.search_masked(qd, 10, 50, md), P.twin.search_masked(P.q, 10, 50, words_of(m & ~S)), (metric, D, "device, masked"))
    assert torch.equal(md, keep)                                                    # the caller's mask is only read
    marked_only(P, np.zeros(P.n, bool))


@pytest.mark.parametrize("M,K", pq_layouts(16))
def test_adc_search_equals_masked_twin(amd, orc, pairs, M, K):
    P = pairs(1, 16)
    opq, _, _, _, _, _ = opq_over_graph(amd, orc, P.blob, 16, M, K)
    rng = np.random.default_rng(M)
    S = rng.random(P.n) < 0.33
    marked_only(P, S)
    m = rng.random(P.n) < 0.5
    w_live, w_m, w_both = words_of(~S), words_of(m, garbage=True), words_of(m & ~S)
    for k, ef in GRID:
        same(P.ix.search_adc(opq, P.q, k, ef), P.twin.search_adc_masked(opq, P.q, k, ef, w_live), (M, k, ef, "adc"))
        same(P.ix.search_adc_masked(opq, P.q, k, ef, w_m), P.twin.search_adc_masked(opq, P.q, k, ef, w_both), (M, k, ef, "adc masked"))
    assert P.ix.last_masked()[3] == 1
    for k, ef, rr in ((5, 40, 40), (10, 64, 30), (1, 16, 8)):
        same(P.ix.search_adc_rerank(opq, P.q, k, ef, rr), P.twin.search_adc_rerank_masked(opq, P.q, k, ef, w_live, rr), (M, k, ef, rr, "rerank"))
        same(P.ix.search_adc_rerank_masked(opq, P.q, k, ef, w_m, rr), P.twin.search_adc_rerank_masked(opq, P.q, k, ef, w_both, rr), (M, k, ef, rr, "rerank masked"))
    opq.close()
    marked_only(P, np.zeros(P.n, bool))


@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_tail_words_and_all_dead(amd, n):
    P = Pair(amd, 1, 8, quarter_rows(n, 8, 70 + n, dup=20), labels=scattered_labels(n, n).view(np.uint64), M=4, nq=16)
    rng = np.random.default_rng(n)
    last = np.zeros(n, bool); last[n - 1] = True
    for name, S in (("third", rng.random(n) < 0.33), ("last node", last), ("all but the last", ~last), ("last word", np.arange(n) >= (n - 1) // 64 * 64)):
        marked_only(P, S)
        assert np.array_equal(P.ix.deleted_mask(), words_of(S)) and np.array_equal(P.ix.deleted_mask(5)[(n + 63) // 64:], np.zeros(5 - (n + 63) // 64, np.uint64))
        m = rng.random(n) < 0.6
        for k, ef in GRID:
            same(P.ix.search(P.q, k, ef), P.twin.search_masked(P.q, k, ef, words_of(~S)), (n, name, k, ef))
            same(P.ix.search_masked(P.q, k, ef, words_of(m, extra=2, garbage=True)), P.twin.search_masked(P.q, k, ef, words_of(m & ~S)), (n, name, k, ef, "masked"))
            same(P.ix.search_masked(P.q, k, ef, words_of(np.ones(n, bool), garbage=True)), P.twin.search_masked(P.q, k, ef, words_of(~S)), (n, name, k, ef, "ones"))
    marked_only(P, np.ones(n, bool))
    zero = P.twin.search_masked(P.q, 10, 50, np.zeros(n, bool))
    assert (zero[1] == -1).all() and not bits(zero[0]).any()
    same(P.ix.search(P.q, 10, 50), zero, (n, "all dead"))
    same(P.ix.search_masked(P.q, 10, 50, words_of(np.ones(n, bool), garbage=True)), zero, (n, "all dead, masked"))
    P.close()


def test_all_dead_pads_the_adc_entries(amd, orc, pairs):
    P = pairs(1, 16)
    opq, _, _, _, _, _ = opq_over_graph(amd, orc, P.blob, 16, 16, 256)
    marked_only(P, np.ones(P.n, bool))
    none = words_of(np.zeros(P.n, bool))
    ones = words_of(np.ones(P.n, bool), garbage=True)
    same(P.ix.search_adc(opq, P.q, 10, 50), P.twin.search_adc_masked(opq, P.q, 10, 50, none), "adc")
    same(P.ix.search_adc_masked(opq, P.q, 10, 50, ones), P.twin.search_adc_masked(opq, P.q, 10, 50, none), "adc masked")
    same(P.ix.search_adc_rerank(opq, P.q, 5, 40, 40), P.twin.search_adc_rerank_masked(opq, P.q, 5, 40, none, 40), "rerank")
    d, lab = P.ix.search_adc_rerank_masked(opq, P.q, 5, 40, ones, 40)
    assert (np.asarray(lab) == -1).all()
    opq.close()
    marked_only(P, np.zeros(P.n, bool))


# ---- 2. state ---------------------------------------------------------------------------------------------------------------------------
def test_state_follows_isin(amd):
    import torch
    n, D = 600, 8
    x = quarter_rows(n, D, 91)
    labels = scattered_labels(n, 9)
    labels[100:110] = labels[:10]                       # labels carried by two nodes
    ix = amd.hnsw_build(x, 1, 4, 32, labels=labels.view(np.uint64), max_batch=1)
    q = mixed_queries(x, 32, 5)
    base = ix.search(q, 10, 50)
    rng = np.random.default_rng(10)
    foreign = np.array([-1, 1 << 62, (1 << 40) + 7], np.int64)
    foreign = foreign[~np.isin(foreign, labels)]
    state = np.zeros(n, bool)
    assert ix.deleted_count() == 0 and not ix.deleted_mask().any()
    picked = labels[rng.random(n) < 0.2]
    steps = [("mark", picked), ("mark", rng.permutation(np.concatenate([picked, picked[:30], foreign]))),     # repeat: changed == 0
             ("mark", labels[:10]), ("mark", np.zeros(0, np.int64)), ("unmark", labels[5:8]), ("unmark", foreign),
             ("unmark", np.zeros(0, np.int64)), ("mark", labels[::-1].copy()), ("mark", labels[:1])]
    for i, (op, s) in enumerate(steps):
        hit = np.isin(labels, s)
        new = state | hit if op == "mark" else state & ~hit
        arg = torch.from_numpy(s).cuda() if i % 2 and s.shape[0] else s
        changed = ix.mark_deleted(arg) if op == "mark" else ix.unmark_deleted(arg)
        assert changed == int((new != state).sum()), (i, op)
        state = new
        assert ix.deleted_count() == int(state.sum()), i
        assert np.array_equal(ix.deleted_mask(), words_of(state)), i
        assert np.array_equal(ix.deleted_mask((n + 63) // 64 + 2), np.concatenate([words_of(state), np.zeros(2, np.uint64)])), i
    assert state.all() and steps[2][1].shape[0] == 10 and state[100:110].all()
    with amd.launch_log() as log:
        ix.search(q, 10, 50)
    assert [r[0] for r in log] == ["hnsw_live_mask_kernel", "hnsw_search_kernel<masked>"]
    assert ix.unmark_deleted(labels) == n and ix.deleted_count() == 0
    with amd.launch_log() as log:
        got = ix.search(q, 10, 50)
    assert [r[0] for r in log] == ["hnsw_search_kernel"]                   # back on the unmasked kernel, and its answers
    same(got, base, "after unmarking everything")
    with amd.launch_log() as log:
        ix.search_masked(q, 10, 50, np.ones(n, bool))
    assert [r[0] for r in log] == ["hnsw_search_kernel<masked>"]
    ix.close()


# ---- 3. files ---------------------------------------------------------------------------------------------------------------------------
def test_files_carry_the_marks(amd, tmp_path, pairs):
    P = pairs(1, 16)
    rng = np.random.default_rng(3)
    S = rng.random(P.n) < 0.3
    dead = np.flatnonzero(S)
    before = saved(P.ix)
    assert np.array_equal(before, np.frombuffer(P.blob, np.uint8))
    marked_only(P, S)
    after = saved(P.ix)
    assert np.array_equal(after, dm.with_marks(P.blob, dead))              # bit 16 of the dead nodes' count words, nothing else
    cli, _ = host_delete(tmp_path, P.blob, P.labels[S], "cli")
    assert np.array_equal(cli, after)                                      # the host CLI's marked file is the handle's
    again = amd.HnswIndex(after.tobytes(), P.metric, P.D)
    assert again.deleted_count() == len(dead) and np.array_equal(again.deleted_mask(), words_of(S))
    assert np.array_equal(saved(again), after)
    for k, ef in GRID:
        same(again.search(P.q, k, ef), P.ix.search(P.q, k, ef), ("loaded", k, ef))
        same(again.search(P.q, k, ef), P.twin.search_masked(P.q, k, ef, words_of(~S)), ("loaded against the twin", k, ef))
    assert again.unmark_deleted(P.labels) == len(dead) and np.array_equal(saved(again), before)
    again.close()
    bad = after.copy()
    per = int(np.frombuffer(bad[24:32].tobytes(), np.uint64)[0])
    bad[96 + 5 * per + 2] |= 2                                             # bit 17 of node 5's count word
    with pytest.raises(amd.CvtmiError) as e:
        amd.HnswIndex(bad.tobytes(), P.metric, P.D)
    assert e.value.code == EINVAL and "corrupt link count" in str(e.value)
    marked_only(P, np.zeros(P.n, bool))


# ---- 4. add on a marked graph -----------------------------------------------------------------------------------------------------------
def add_and_compare(amd, orc, tmp_path, marked, metric, D, extra, labels, tag, batches=(2, 7, 0), cont=False, need=None):
    """cvtmi_hnsw_add of `extra` on a handle loaded from the file `marked`: max_batch = 1 against the host mirror's file, the batched
    schedules against the model's; returns the model's counters per batch size"""
    n0 = parse(marked)["cnt"]
    host = host_add(tmp_path, marked, extra, D, metric, tag, labels=labels, cont=cont)
    levels = parse(host)["levels"][n0:]
    dead = dm.dead_of(marked)
    counters = {}
    for b in (1,) + tuple(batches):
        want, cnt = dm.add_model(orc, marked, metric, extra, levels, labels, b)
        counters[b] = cnt
        if need:
            need(b, cnt)
        idx = amd.HnswIndex(marked.tobytes(), metric, D)
        if cont:
            idx.set_level_draws(n0)
        with amd.launch_log() as log:
            idx.add(extra, labels, max_batch=b)
        names = {r[0] for r in log if r[0].startswith("hnsw_build_search_kernel")}
        assert names == ({"hnsw_build_search_kernel<del>"} if len(dead) else {"hnsw_build_search_kernel"}), (tag, b, names)
        got = saved(idx)
        assert got.size == want.size and np.array_equal(got, want), (tag, b, cnt)
        if b == 1:
            assert np.array_equal(got, host), (tag, "host mirror")
        assert idx.deleted_count() == len(dead) and np.array_equal(idx.deleted_mask(), words_of(np.isin(np.arange(n0 + len(extra)), dead)))
        idx.close()
    return counters


@pytest.mark.parametrize("which", DEAD_SETS)
@pytest.mark.parametrize("metric,D", SHAPES)
def test_add_on_a_marked_graph_is_the_model(amd, orc, tmp_path, pairs, metric, D, which):
    """every DEL instance of the construction traversal (<IP,1> <IP,4> <L2,1> <L2,4> <L2,8>) under the five dead sets"""
    P = pairs(metric, D)
    dead = dead_set(which, P.g)
    marked = dm.with_marks(P.blob, dead)
    extra = extra_rows(P.g, 60, 100 + D)
    labels = np.arange(60, dtype=np.uint64) + 10 ** 7
    cnt = add_and_compare(amd, orc, tmp_path, marked, metric, D, extra, labels, "%d_%d_%s" % (metric, D, which))
    print(metric, D, which, cnt)
    assert cnt[0]["largest_batch"] > 7                                     # the default schedule: N // 32 rows
    if which == "none":                                                    # today's bytes
        ref = amd.HnswIndex(P.blob, metric, D)
        ref.add(extra, labels, max_batch=7)
        want, _ = dm.add_model(orc, np.frombuffer(P.blob, np.uint8), metric, extra, parse(saved(ref))["levels"][P.n:], labels, 7, dead=[])
        assert np.array_equal(saved(ref), want)
        ref.close()


def test_add_with_a_dead_hub(amd, orc, tmp_path):
    """inner product, one row far out that is every row's nearest node, dead: it is walked through by every insertion and never linked"""
    n, D = 600, 8
    x = hm._hub(n + 50, D, 8)
    base = amd.hnsw_build(x[:n], 0, 4, 16, max_batch=1)
    blob = saved(base)
    base.close()
    g = parse(blob)
    assert (g["l0"][:, 1:] == 3).any(axis=1).sum() > n // 4                # the hub: a quarter of the graph links to it
    marked = dm.with_marks(blob, [3])
    cnt = add_and_compare(amd, orc, tmp_path, marked, 0, D, x[n:], None, "hub")
    print("hub", cnt)
    out = parse(dm.add_model(orc, marked, 0, x[n:], parse(host_add(tmp_path, marked, x[n:], D, 0, "hub_lv"))["levels"][n:], None, 7)[0])
    for row in out["l0"][n:]:
        assert 3 not in row[1:1 + (row[0] & 0xffff)] or g["ep"] == 3
    # the hub and all but 12 other nodes dead, efc = 16: the result queues cannot fill, so no walk may stop before its candidate
    # queue is empty -- it runs on past candidates beyond `lower`, through the hub, with a result queue of at most 12 entries
    live = np.random.default_rng(2).choice(np.setdiff1d(np.arange(n), [3]), 12, replace=False)

    def need(b, c):
        assert c["past_stop"] > 0 and c["cand_max"] > 16, (b, c)
    cnt = add_and_compare(amd, orc, tmp_path, dm.with_marks(blob, np.setdiff1d(np.arange(n), live)), 0, D, x[n:], None, "hub_few", need=need)
    print("hub, 12 live", cnt)


def test_add_raises_the_top_level_past_a_dead_entry_point(amd, orc, tmp_path):
    """M = 2: row 115 of the level stream rises above everything before it.  The graph of the first 100 rows has its entry point
    deleted; the add continues the stream (set_level_draws), so row 115 becomes the live entry point of the rows behind it."""
    x = hm._normal(140, 24, 78)
    base = amd.hnsw_build(x[:100], 1, 2, 16, max_batch=1)
    blob = saved(base)
    base.close()
    g = parse(blob)
    marked = dm.with_marks(blob, [g["ep"]])

    def need(b, cnt):
        assert cnt["ep_pushes"] > 0
    add_and_compare(amd, orc, tmp_path, marked, 1, 24, x[100:], None, "rise", cont=True, need=need)
    out = parse(host_add(tmp_path, marked, x[100:], 24, 1, "rise_chk", cont=True))
    assert out["ep"] == 115 and out["maxlevel"] > g["maxlevel"] and out["l0"][g["ep"], 0] >> 16 == 1


def test_add_across_bitmap_words_and_a_storage_doubling(amd, orc, tmp_path):
    """63 nodes + 70 rows: the bitmap grows from one word to three, device storage more than doubles; old marks stay, new rows are live"""
    n, D = 63, 8
    x = quarter_rows(n + 70, D, 63, dup=20)
    base = amd.hnsw_build(x[:n], 1, 4, 32, max_batch=1)
    blob = saved(base)
    g = parse(blob)
    dead = np.union1d(dead_set("third", g), [62])
    add_and_compare(amd, orc, tmp_path, dm.with_marks(blob, dead), 1, D, x[n:], None, "grow")
    # the same on the handle that was built, marked through the ABI, in two calls (64 is crossed by the first, 128 by the second)
    base.mark_deleted(g["labels"][dead])
    base.add(x[n:n + 30], max_batch=1)
    base.add(x[n + 30:], max_batch=1)
    S = np.isin(np.arange(n + 70), dead)
    assert base.deleted_count() == len(dead) and np.array_equal(base.deleted_mask(), words_of(S))
    q = mixed_queries(x, 16, 3)
    twin = amd.HnswIndex(dm.with_marks(saved(base), dead, on=False).tobytes(), 1, D)
    same(base.search(q, 10, 50), twin.search_masked(q, 10, 50, words_of(~S)), "grown")
    assert base.mark_deleted(np.array([n + 69], np.int64)) == 1 and base.deleted_count() == len(dead) + 1      # default labels: the ids
    twin.close()
    base.close()


def test_candidate_queue_past_the_bound_without_deletions(amd, orc, tmp_path):
    """1500 nodes, 8 of them live, M = 4, efc = 16: the walks find fewer than efc live nodes, nothing is pruned, and the candidate
    queue holds up to 540 entries (model, CPU) where the construction without deletions reserves max(256, min(2 efc maxM0, n)) + 64
    = 320; walks run on past the first candidate beyond `lower`.  The file is still the model's: no overflow."""
    n, D, M, efc = 1500, 8, 4, 16
    x = np.random.default_rng(n + D).normal(size=(n + 12, D)).astype(np.float32)
    base = amd.hnsw_build(x[:n], 1, M, efc, max_batch=1)
    blob = saved(base)
    base.close()
    dead = np.setdiff1d(np.arange(n), np.random.default_rng(1).choice(n, 8, replace=False))
    reserved = max(256, min(2 * efc * 2 * M, n)) + 64

    def need(b, cnt):
        assert cnt["cand_max"] > reserved and cnt["past_stop"] > 0, (b, cnt)
    cnt = add_and_compare(amd, orc, tmp_path, dm.with_marks(blob, dead), 1, D, x[n:], None, "queue", batches=(7,), need=need)
    print("queue bound: reserved %d without deletions, model %s" % (reserved, cnt))


def test_add_without_deletions_launches_what_it_launched(amd, pairs):
    """n_dead == 0, after marks that were all taken back too: no <del> kernel, no mask kernel"""
    P = pairs(1, 20)
    extra = extra_rows(P.g, 40, 9)
    idx = amd.HnswIndex(P.blob, 1, 20)
    idx.mark_deleted(P.labels[:50])
    idx.unmark_deleted(P.labels[:50])
    with amd.launch_log() as log:
        idx.add(extra, max_batch=7)
    names = [r[0] for r in log]
    assert "hnsw_build_search_kernel" in names and not [s for s in names if "del" in s or "mask" in s or "dead" in s], names
    fresh = amd.HnswIndex(P.blob, 1, 20)
    fresh.add(extra, max_batch=7)
    assert np.array_equal(saved(idx), saved(fresh))
    idx.close()
    fresh.close()


# ---- 5. robustness ----------------------------------------------------------------------------------------------------------------------
def test_argument_checks_leave_the_handle_usable(amd, pairs):
    P = pairs(1, 16)
    lib = amd.lib()
    h = P.ix.h
    S = np.zeros(P.n, bool); S[:100] = True
    marked_only(P, S)
    want = P.ix.search(P.q, 10, 50)
    lab = np.ascontiguousarray(P.labels[:4])
    p = lambda a: C.c_void_p(a.ctypes.data)
    null = C.c_void_p(0)
    ch = C.c_int64(-7)
    mask = np.zeros((P.n + 63) // 64, np.uint64)
    assert lib.cvtmi_hnsw_mark_deleted(h, p(lab), C.c_int64(-1), C.byref(ch)) == EINVAL
    assert lib.cvtmi_hnsw_mark_deleted(h, null, C.c_int64(3), C.byref(ch)) == EINVAL
    assert lib.cvtmi_hnsw_unmark_deleted(h, null, C.c_int64(3), null) == EINVAL
    assert lib.cvtmi_hnsw_unmark_deleted_dev(h, p(lab), C.c_int64(-2), null, null) == EINVAL
    assert lib.cvtmi_hnsw_get_deleted(h, p(mask), C.c_int64(mask.shape[0] - 1)) == EINVAL and b"mask words" in lib.cvtmi_last_error()
    assert lib.cvtmi_hnsw_get_deleted(h, null, C.c_int64(mask.shape[0])) == EINVAL
    assert lib.cvtmi_hnsw_get_deleted(h, p(mask), C.c_int64(-1)) == EINVAL
    assert lib.cvtmi_hnsw_deleted_count(h, null) == EINVAL
    assert ch.value == -7
    assert lib.cvtmi_hnsw_mark_deleted(h, null, C.c_int64(0), C.byref(ch)) == 0 and ch.value == 0            # an empty set does nothing
    assert lib.cvtmi_hnsw_mark_deleted(h, p(lab), C.c_int64(4), null) == 0                                    # changed may be NULL
    assert P.ix.deleted_count() == 100 and np.array_equal(P.ix.deleted_mask(), words_of(S))
    same(P.ix.search(P.q, 10, 50), want, "after the refusals")
    marked_only(P, np.zeros(P.n, bool))


def test_four_threads_search_a_marked_handle(amd, pairs):
    P = pairs(1, 16)
    rng = np.random.default_rng(77)
    S = rng.random(P.n) < 0.4
    marked_only(P, S)
    m = words_of(rng.random(P.n) < 0.5)
    jobs = [("unmasked", lambda: P.ix.search(P.q, 10, 50)), ("masked", lambda: P.ix.search_masked(P.q, 20, 20, m)),
            ("unmasked small", lambda: P.ix.search(P.q[:5], 3, 16)), ("count", lambda: (np.array([P.ix.deleted_count()], np.float32), P.ix.deleted_mask().view(np.int64)))]
    want = {name: fn() for name, fn in jobs}
    same(want["unmasked"], P.twin.search_masked(P.q, 10, 50, words_of(~S)), "alone")
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
    marked_only(P, np.zeros(P.n, bool))


def test_cli_delete_then_search(amd, tmp_path, pairs):
    """hnsw_delete followed by hnsw_search == mark_deleted followed by search"""
    P = pairs(1, 16)
    rng = np.random.default_rng(8)
    S = rng.random(P.n) < 0.25
    marked, _ = host_delete(tmp_path, P.blob, P.labels[S], "cli_search")
    (tmp_path / "g.hnsw").write_bytes(marked.tobytes())
    (tmp_path / "q.bin").write_bytes(P.q.tobytes())
    k, ef = 10, 50
    r = subprocess.run([os.path.join(BIN, "hnsw_search"), "g.hnsw", "q.bin", "16", str(k), str(ef), "out.txt", "l2"], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    marked_only(P, S)
    d, lab = P.ix.search(P.q, k, ef)
    lines = (tmp_path / "out.txt").read_text().splitlines()
    assert len(lines) == P.q.shape[0]
    for qi, line in enumerate(lines):
        pairs_ = [t.split(":") for t in line.split()]
        cnt = len(pairs_)
        assert [int(t[0]) for t in pairs_] == lab[qi, :cnt].tolist() and (lab[qi, cnt:] == -1).all(), qi
        assert np.array_equal(bits(np.array([float(t[1]) for t in pairs_], np.float32)), bits(d[qi, :cnt])), qi
    assert not np.isin(lab[lab >= 0], P.labels[S]).any()
    marked_only(P, np.zeros(P.n, bool))
