"""The batch-synchronous HNSW build (cvtmi_hnsw_build) restated in plain Python, and the table of shapes that
test_hnsw_build_model.py (CPU: the model against files the reference and the host mirror wrote, and each shape against the path
it is there for) and test_gpu_hnsw_build_batches.py (GPU: the built file against the model's, byte for byte) share.

The insertion is the host mirror's (cvt_amd/host/hnswlib/hnswalg.h: insert, search_level, select, connect), one statement at a
time; what DESIGN 4.11 adds is the schedule, "every row of a batch sees the graph as the batch found it", and the order in which
a batch's back links are applied.  Nothing here is taken from csrc/hnsw_build.hip.

Distances are the oracle's (orc.dist, flavour 4), memoised per unordered pair: both metrics are symmetric bit for bit (a * b and
(a - b)^2 commute).  `vectorised=True` computes one node's distances to every row with numpy instead, in the oracle's summation
order; test_hnsw_build_model.py shows the two bit-equal, in both argument orders, for every (metric, D) used.  NaN rows are out
of scope (std::priority_queue has no defined behaviour on them)."""
import ctypes as C
import math
import struct

import numpy as np

from test_gpu_hnsw_build import tie_heavy
from test_gpu_hnsw_edges import pop_heap, push_heap

ROW_CACHE_FLOATS = 12_000_000   # vectorised distances: Python floats kept at most (rows of n floats each)


def dist_row(x, metric, i):
    """distances of row i to every row of x [n][D] (float32), in orc.dist's order for flavour 4: scalar for D % 4 != 0, else 4
    lanes (8 for L2 and D % 16 == 0), every accumulator starting from +0, lanes added left to right"""
    n, D = x.shape
    lanes = 1 if D % 4 else 4 if metric == 0 else 8 if D % 16 == 0 else 4
    xt = np.ascontiguousarray(x.T)
    a = x[i]
    acc = np.zeros((lanes, n), np.float32)
    for k in range(D):
        if metric == 0:
            t = xt[k] * a[k]
        else:
            t = a[k] - xt[k]
            t = t * t
        acc[k % lanes] += t
    s = acc[0]
    for lane in range(1, lanes):
        s = s + acc[lane]
    return np.float32(1.0) - s if metric == 0 else s


class _OracleRow:
    """d(i, .) one pair at a time: orc.dist(metric, 4, x[i], x[j]), called on the rows where they lie (orc.dist itself converts both
    arrays on every call, which is most of its time)"""

    def __init__(self, owner, i):
        self.owner, self.i = owner, i

    def __getitem__(self, j):
        o, i = self.owner, self.i
        key = (i, j) if i < j else (j, i)
        d = o.memo.get(key)
        if d is None:
            d = o.memo[key] = float(o.fn(o.metric, 4, C.c_void_p(o.base + i * o.stride), C.c_void_p(o.base + j * o.stride), o.D))
        return d


class Distances:
    """row(i)[j] = d(i, j) as a Python float"""

    def __init__(self, orc, x, metric, vectorised):
        self.x, self.metric, self.vectorised = x, metric, vectorised
        self.memo, self.rows = {}, {}
        self.fn, self.base, self.stride, self.D = orc.lib.orc_dist, x.ctypes.data, x.strides[0], x.shape[1]
        assert x.flags.c_contiguous and x.dtype == np.float32 and self.fn.restype is C.c_float

    def row(self, i):
        r = self.rows.get(i)
        if r is None:
            if self.vectorised:
                if (len(self.rows) + 1) * self.x.shape[0] > ROW_CACHE_FLOATS:
                    self.rows.clear()
                r = dist_row(self.x, self.metric, i).tolist()
            else:
                r = _OracleRow(self, i)
            self.rows[i] = r
        return r


def schedule(levels, n, max_batch, frac=32, cap=8192):
    """[(first, end, entry point, top level, cut)] of every batch after the seed row: a batch holds max(1, inserted // frac) rows,
    at most max_batch (cap when max_batch == 0), and ends with the first row whose level exceeds the top level; `cut` says that
    this row was not the last of the planned batch anyway"""
    limit = max_batch if max_batch > 0 else cap
    out, s, top, ep = [], 1, int(levels[0]), 0
    while s < n:
        planned = min(s + min(max(1, s // frac), limit), n)
        e, cut = planned, False
        for i in range(s, planned):
            if levels[i] > top:
                e, cut = i + 1, i + 1 < planned
                break
        out.append((s, e, ep, top, cut))
        if levels[e - 1] > top:
            ep, top = e - 1, int(levels[e - 1])
        s = e
    return out


def build_model(orc, x, metric, M, efc, levels, labels, max_batch, frac=32, cap=8192, vectorised=False):
    """-> (the saveIndex file as bytes, counters).  levels[i] = the level drawn for row i (from a file the host mirror or the
    reference wrote), labels = None for the row numbers.  Counters, per build:
      props_l0, props_up     most proposals one (target, level) received in one batch, on level 0 / on a level >= 1
      reselect_max           most re-selections of one full list inside one batch
      shortened              re-selections that shortened a list
      shortened_then_append  of those, followed in the same batch by an append into the freed word
      multi_level_targets    (target, batch) pairs with proposals on two or more levels
      raised, cut_batches, cut_rise2     rows that raised the top level; those that were not the last row of their planned batch;
                             of those, rises by two or more levels
      short_queues           rows, in batches of more than one row, with a result queue below M on some level
      props_target           most proposals one target received in one batch, over all levels
      tie_runs               heuristic runs whose candidates held two equal distances under different ids
      reselect65             re-selections over 65 candidates
      batches, largest_batch the seed row counts as batch 0
      touched[(node, level)] the index of the last batch that wrote that list"""
    x = np.ascontiguousarray(x, np.float32)
    n, D = x.shape
    levels = [int(v) for v in levels]
    assert len(levels) == n and n >= 1
    labels = np.arange(n, dtype=np.uint64) if labels is None else np.ascontiguousarray(labels).view(np.uint64)
    efc = max(efc, M)
    maxM, maxM0 = M, 2 * M
    dist = Distances(orc, x, metric, vectorised)
    # every list is [count, word 1 .. word room]; all words start as zeros (insert: std::fill / assign)
    l0 = [[0] * (maxM0 + 1) for _ in range(n)]
    up = [[[0] * (maxM + 1) for _ in range(levels[i])] for i in range(n)]

    def links(i, l):
        return l0[i] if l == 0 else up[i][l - 1]

    cnt = dict(batches=1, props_l0=0, props_up=0, reselect_max=0, shortened=0, shortened_then_append=0, multi_level_targets=0,
               raised=0, cut_batches=0, cut_rise2=0, short_queues=0, props_target=0, tie_runs=0, reselect65=0, largest_batch=1,
               touched={(0, l): 0 for l in range(levels[0] + 1)})
    touched = cnt["touched"]

    def search_level(start, di, l):
        best, frontier = [], []
        d0 = di[start]
        push_heap(best, (d0, start))
        push_heap(frontier, (-d0, start))
        seen = {start}
        bound = d0
        while frontier:
            c = frontier[0]
            if -c[0] > bound:
                break
            pop_heap(frontier)
            w = links(c[1], l)
            for j in range(1, 1 + w[0]):
                nb = w[j]
                if nb in seen:
                    continue
                seen.add(nb)
                d = di[nb]
                if best[0][0] > d or len(best) < efc:
                    push_heap(frontier, (-d, nb))
                    push_heap(best, (d, nb))
                    if len(best) > efc:
                        pop_heap(best)
                    bound = best[0][0]
        return best

    def select(cands, m):
        """getNeighborsByHeuristic2: untouched below m candidates; else nearest first (equal distances by decreasing id, +0 = -0),
        a candidate is kept when no kept one is closer to it than the query point is; the kept pairs pushed into a heap"""
        if len(cands) < m:
            return cands
        order = sorted(cands, key=lambda c: (c[0], -c[1]))
        if any(order[j][0] == order[j + 1][0] for j in range(len(order) - 1)):
            cnt["tie_runs"] += 1
        kept, kept_rows = [], []
        for c in order:
            if len(kept) >= m:
                break
            to_query, node = c
            ok = True
            for r in kept_rows:
                if r[node] < to_query:
                    ok = False
                    break
            if ok:
                kept.append(c)
                kept_rows.append(dist.row(node))
        out = []
        for c in kept:
            push_heap(out, c)
        return out

    def drain(heap):
        out = []
        while heap:
            out.append(heap[0][1])
            pop_heap(heap)
        return out

    for b, (s, e, ep, top, cut) in enumerate(schedule(levels, n, max_batch, frac, cap), 1):
        cnt["batches"] += 1
        cnt["largest_batch"] = max(cnt["largest_batch"], e - s)
        if levels[e - 1] > top:
            cnt["raised"] += 1
            if cut:
                cnt["cut_batches"] += 1
                cnt["cut_rise2"] += levels[e - 1] - top >= 2
        own, props = [], {}
        # ---- every row against the graph as the batch found it
        for i in range(s, e):
            lvl = levels[i]
            di = dist.row(i)
            cur = ep
            if lvl < top:
                cd = di[cur]
                for l in range(top, lvl, -1):
                    moved = True
                    while moved:
                        moved = False
                        w = links(cur, l)
                        for j in range(1, 1 + w[0]):
                            d = di[w[j]]
                            if d < cd:
                                cd, cur, moved = d, w[j], True
            short = False
            for l in range(min(lvl, top), -1, -1):   # every level starts from the same node
                found = search_level(cur, di, l)
                short = short or len(found) < M
                chosen = drain(select(found, M))
                assert len(chosen) <= M and i not in chosen
                own.append((i, l, chosen))
                for t in chosen:
                    assert levels[t] >= l
                    props.setdefault((t, l), []).append(i)
            if short and e - s > 1:
                cnt["short_queues"] += 1
        for i, l, chosen in own:
            w = links(i, l)
            w[1:1 + len(chosen)] = chosen
            w[0] = len(chosen)
        for i in range(s, e):
            for l in range(levels[i] + 1):
                touched[(i, l)] = b
        # ---- back links, per target in increasing (level, source id)
        per_target = {}
        for (t, l) in sorted(props):
            src = props[(t, l)]
            assert src == sorted(src)
            per_target.setdefault(t, []).append(len(src))
            key = "props_l0" if l == 0 else "props_up"
            cnt[key] = max(cnt[key], len(src))
            touched[(t, l)] = b
            w = links(t, l)
            room = maxM0 if l == 0 else maxM
            rt = dist.row(t)
            reselections, freed = 0, False
            for new in src:
                have = w[0]
                if have < room:
                    w[1 + have] = new
                    w[0] = have + 1
                    if freed:
                        cnt["shortened_then_append"] += 1
                        freed = False
                    continue
                pool = [(rt[new], new)] + [(rt[w[1 + j]], w[1 + j]) for j in range(have)]
                cnt["reselect65"] += len(pool) == 65
                kept = drain(select(pool, room))
                w[1:1 + len(kept)] = kept     # words past a shortened list keep what they held
                w[0] = len(kept)
                reselections += 1
                if len(kept) < room:
                    cnt["shortened"] += 1
                    freed = True
            cnt["reselect_max"] = max(cnt["reselect_max"], reselections)
        for t, sizes in per_target.items():
            cnt["multi_level_targets"] += len(sizes) >= 2
            cnt["props_target"] = max(cnt["props_target"], sum(sizes))

    # ---- the reference's saveIndex image
    top, ep = levels[0], 0
    for i in range(1, n):
        if levels[i] > top:
            top, ep = levels[i], i
    per = 4 + 4 * maxM0 + 4 * D + 8
    head = struct.pack("<6QiI3QdQ", 0, n, n, per, 4 + 4 * maxM0 + 4 * D, 4 + 4 * maxM0, top, ep, maxM, maxM0, M, 1 / math.log(1.0 * M), efc)
    body = np.zeros((n, per), np.uint8)
    body[:, :4 + 4 * maxM0] = np.array(l0, dtype=np.uint32).view(np.uint8)
    body[:, 4 + 4 * maxM0:per - 8] = x.view(np.uint8)
    body[:, per - 8:] = labels.reshape(n, 1).view(np.uint8)
    tail = []
    for i in range(n):
        tail.append(struct.pack("<I", (4 * maxM + 4) * levels[i]))
        if levels[i]:
            tail.append(np.array(up[i], dtype=np.uint32).tobytes())
    return head + body.tobytes() + b"".join(tail), cnt


def first_difference(got, want, cnt):
    """the first (node, level) whose words differ between two parsed files (test_gpu_hnsw_build.parse), both lists as stored (all
    words), and the model's last batch that touched it; None when all link words agree"""
    for i in range(want["cnt"]):
        if not np.array_equal(got["l0"][i], want["l0"][i]):
            return (i, 0), got["l0"][i].tolist(), want["l0"][i].tolist(), cnt["touched"].get((i, 0))
        for l in range(1, int(want["levels"][i]) + 1):
            a, b = got["upper"].get((i, l)), want["upper"][(i, l)]
            if a is None or not np.array_equal(a, b):
                return (i, l), None if a is None else a.tolist(), b.tolist(), cnt["touched"].get((i, l))
    return None


# ---- the shapes -------------------------------------------------------------------------------------------------------------------
def _normal(n, D, seed):
    return np.random.default_rng(seed).normal(size=(n, D)).astype(np.float32)


def _hub(n, D, seed):
    """log-normal row norms, every row on one side of a hyperplane, and one row far out on that side, inserted early: under the
    inner product it is every later row's nearest node"""
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(n, D)) * np.exp(0.5 * rng.normal(size=(n, 1)))).astype(np.float32)
    x[:, 0] = np.abs(x[:, 0]) + np.float32(0.25)
    x[3] = 0
    x[3, 0] = 200
    return x


def _identical(n, D, seed):
    return np.repeat(np.random.default_rng(seed).normal(size=(1, D)).astype(np.float32), n, axis=0)


def _labels(n):
    return np.arange(n, dtype=np.uint64) * 7 + 3


# name: metric, rows, M, efc, max_batch, frac, labels, conditions on the model's counters
CASES = {
    "A-2": dict(metric=1, rows=lambda: _normal(1500, 16, 11), M=6, efc=30, max_batch=2, need=lambda c: c["largest_batch"] == 2),
    "A-7": dict(metric=1, rows=lambda: _normal(1500, 16, 11), M=6, efc=30, max_batch=7, need=lambda c: c["largest_batch"] == 7),
    "A-64": dict(metric=1, rows=lambda: _normal(1500, 16, 11), M=6, efc=30, max_batch=64, need=lambda c: c["props_l0"] >= 3),
    "A-0": dict(metric=1, rows=lambda: _normal(1500, 16, 11), M=6, efc=30, max_batch=0, need=lambda c: c["props_l0"] >= 3),
    "B": dict(metric=0, rows=lambda: tie_heavy(1200, 20, 20), M=8, efc=40, max_batch=0, frac=2, labels=_labels, device=True,
              need=lambda c: c["props_l0"] >= 3 and c["props_up"] >= 3 and c["reselect_max"] >= 2 and c["multi_level_targets"] >= 1
              and c["tie_runs"] >= 1),
    "C": dict(metric=1, rows=lambda: _normal(800, 7, 7), M=4, efc=20, max_batch=0, frac=1,
              need=lambda c: c["reselect_max"] >= 2 and c["shortened"] >= 1 and c["shortened_then_append"] >= 1
              and c["short_queues"] >= 1),
    "D": dict(metric=0, rows=lambda: _normal(1000, 10, 10), M=32, efc=32, max_batch=0, frac=2,
              need=lambda c: c["reselect65"] >= 1 and c["short_queues"] >= 1),
    "E": dict(metric=0, rows=lambda: _hub(8300, 8, 8), M=4, efc=16, max_batch=0, frac=1, need=lambda c: c["props_target"] > 2048),
    # levels are draws of one fixed engine scaled by 1 / ln M: no choice of rows or seed moves them.  At M = 4 no row of the first
    # 4000 rises two levels at once; at M = 2 row 115 goes from 6 to 9, in the middle of a batch of three
    "F": dict(metric=1, rows=lambda: _normal(3000, 24, 77), M=4, efc=16, max_batch=64, need=lambda c: c["cut_batches"] >= 1),
    "F-rise2": dict(metric=1, rows=lambda: _normal(700, 24, 78), M=2, efc=16, max_batch=64,
                    need=lambda c: c["cut_batches"] >= 1 and c["cut_rise2"] >= 1),
    "G": dict(metric=0, rows=lambda: _identical(300, 16, 77), M=8, efc=20, max_batch=7, need=lambda c: c["tie_runs"] >= 1),
}
