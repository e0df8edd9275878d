"""cvtmi_hnsw_add on a graph with deleted nodes restated in plain Python: a saveIndex file, a dead set and new rows in,
the file after the add out.  A helper, not a test; tests/test_host_hnsw_delete.py holds the host mirror's addPoint to it on the CPU,
tests/test_gpu_hnsw_delete.py the device's files, byte for byte.

The rule (current hnswlib's addPoint / searchBaseLayer on a graph with marked nodes, stated in DESIGN 4.7.2):
  * the greedy descent walks dead nodes like live ones;
  * on a level, the entry joins the candidate queue and is visited either way; live, it also joins the result queue and `lower` is its
    distance; dead, the result queue stays empty and `lower` is +inf;
  * an unvisited neighbour at distance d is accepted while the result queue holds fewer than efc entries, or when lower > d; accepted,
    it joins the candidate queue, and the result queue only if it is live (popped past efc); `lower` follows the result queue's
    maximum once that holds something;
  * the walk stops on -c.d > lower only when the result queue holds efc entries;
  * after the walk, if the batch's entry point is dead, (d(row, entry point), entry point) is pushed into the level's result queue,
    which is popped if it then exceeds efc.
Selection, the row's own list and the back links are the build's (tests/hnsw_build_model.py), dead members treated like any other.

The heaps, the distances and the schedule are those of tests/hnsw_build_model.py; the insertion loop is restated because that file's
loop is closed over a build from row 0.  The dead bit of a node is bit 16 of its level-0 count word in the file, in and out."""
import struct

import numpy as np

import hnsw_build_model as hm
from test_gpu_hnsw_build import parse
from test_gpu_hnsw_edges import pop_heap, push_heap
from test_host_hnsw_add import build_then_add_schedule

DELETE_BIT = 1 << 16
INF = float("inf")


def dead_of(blob):
    """the nodes a saveIndex file marks deleted, ascending"""
    p = parse(blob)
    return np.flatnonzero(p["l0"][:, 0] & DELETE_BIT)


def with_marks(blob, dead, on=True):
    """the file `blob` with bit 16 of the level-0 count word of every node in `dead` set (on) or cleared"""
    blob = np.frombuffer(bytes(blob), dtype=np.uint8).copy()
    per = struct.unpack("<Q", blob[24:32].tobytes())[0]
    for i in dead:
        w = blob[96 + int(i) * per:96 + int(i) * per + 4].view(np.uint32)
        w[0] = (w[0] | DELETE_BIT) if on else (w[0] & ~np.uint32(DELETE_BIT))
    return blob


def add_model(orc, blob, metric, x_new, levels_new, labels_new, max_batch, dead=None, frac=32, cap=8192, vectorised=True):
    """-> (the file after cvtmi_hnsw_add(x_new, labels_new, max_batch) on the graph of `blob`, counters).  dead: the deleted nodes
    (None: those the file marks).  levels_new: the levels drawn for the new rows.  Counters:
      cand_max     the longest candidate queue of any walk
      past_stop    walks that ran on past a candidate with -c.d > lower because the result queue was not full
      ep_pushes    entry-point pushes after a walk
      empty_walks  walks that ended with an empty result queue (before the entry-point push)
      batches, largest_batch"""
    p = parse(blob)
    n0, maxM, maxM0, M, D = p["cnt"], p["maxM"], p["maxM0"], p["M"], p["D"]
    mult, efc = struct.unpack("<dQ", np.asarray(blob[80:96]).tobytes())
    assert n0 >= 1
    dead = set(int(i) for i in (dead_of(blob) if dead is None else dead))
    assert all(0 <= i < n0 for i in dead)
    x = np.ascontiguousarray(np.concatenate([p["rows"], np.asarray(x_new, np.float32).reshape(-1, D)]))
    n = x.shape[0]
    levels = [int(v) for v in p["levels"]] + [int(v) for v in levels_new]
    assert len(levels) == n
    labels = np.concatenate([p["labels"], np.arange(n0, n, dtype=np.uint64) if labels_new is None
                             else np.ascontiguousarray(labels_new).view(np.uint64)])
    dist = hm.Distances(orc, x, metric, vectorised)
    l0 = [[int(v) for v in row] for row in p["l0"]] + [[0] * (maxM0 + 1) for _ in range(n - n0)]
    for row in l0[:n0]:
        row[0] &= 0xffff
    up = [[[int(v) for v in p["upper"][(i, l)]] for l in range(1, levels[i] + 1)] for i in range(n0)]
    up += [[[0] * (maxM + 1) for _ in range(levels[i])] for i in range(n0, n)]

    def links(i, l):
        return l0[i] if l == 0 else up[i][l - 1]

    cnt = dict(cand_max=0, past_stop=0, ep_pushes=0, empty_walks=0, batches=0, largest_batch=0)

    def search_level(start, di, l):
        best, frontier = [], []
        d0 = di[start]
        bound = INF
        if start not in dead:
            push_heap(best, (d0, start))
            bound = d0
        push_heap(frontier, (-d0, start))
        seen = {start}
        passed = False
        while frontier:
            c = frontier[0]
            if -c[0] > bound:
                if len(best) >= efc:
                    break
                passed = True
            pop_heap(frontier)
            w = links(c[1], l)
            for j in range(1, 1 + w[0]):
                nb = w[j]
                if nb in seen:
                    continue
                seen.add(nb)
                d = di[nb]
                if len(best) < efc or bound > d:
                    push_heap(frontier, (-d, nb))
                    cnt["cand_max"] = max(cnt["cand_max"], len(frontier))
                    if nb not in dead:
                        push_heap(best, (d, nb))
                        if len(best) > efc:
                            pop_heap(best)
                    if best:
                        bound = best[0][0]
        cnt["past_stop"] += passed
        cnt["empty_walks"] += not best
        return best

    def select(cands, m):
        if len(cands) < m:
            return cands
        order = sorted(cands, key=lambda c: (c[0], -c[1]))
        kept, kept_rows = [], []
        for c in order:
            if len(kept) >= m:
                break
            to_query, node = c
            if all(not (r[node] < to_query) for r in kept_rows):
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

    plan = [b for b in build_then_add_schedule(n0, 1, max_batch)(levels, n, max_batch, frac, cap) if b[0] >= n0]
    if plan:
        assert plan[0][0] == n0 and (plan[0][2], plan[0][3]) == (p["ep"], p["maxlevel"]), "the file's entry point is not the first row of its top level"
    for s, e, ep, top, cut in plan:
        cnt["batches"] += 1
        cnt["largest_batch"] = max(cnt["largest_batch"], e - s)
        own, props = [], {}
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
            for l in range(min(lvl, top), -1, -1):
                found = search_level(cur, di, l)
                if ep in dead:
                    push_heap(found, (di[ep], ep))
                    if len(found) > efc:
                        pop_heap(found)
                    cnt["ep_pushes"] += 1
                chosen = drain(select(found, M))
                assert len(chosen) <= M and i not in chosen and len(set(chosen)) == len(chosen)
                own.append((i, l, chosen))
                for t in chosen:
                    assert levels[t] >= l
                    props.setdefault((t, l), []).append(i)
        for i, l, chosen in own:
            w = links(i, l)
            w[1:1 + len(chosen)] = chosen
            w[0] = len(chosen)
        for (t, l) in sorted(props):
            w = links(t, l)
            room = maxM0 if l == 0 else maxM
            rt = dist.row(t)
            for new in props[(t, l)]:
                have = w[0]
                if have < room:
                    w[1 + have] = new
                    w[0] = have + 1
                    continue
                pool = [(rt[new], new)] + [(rt[w[1 + j]], w[1 + j]) for j in range(have)]
                kept = drain(select(pool, room))
                w[1:1 + len(kept)] = kept
                w[0] = len(kept)

    top, ep = p["maxlevel"], p["ep"]
    for i in range(n0, n):
        if levels[i] > top:
            top, ep = levels[i], i
    per = 4 + 4 * maxM0 + 4 * D + 8
    cap_out = max(p["cap"], n)
    head = struct.pack("<6QiI3QdQ", 0, cap_out, n, per, 4 + 4 * maxM0 + 4 * D, 4 + 4 * maxM0, top, ep, maxM, maxM0, M, mult, efc)
    for i in dead:
        l0[i][0] |= DELETE_BIT
    body = np.zeros((cap_out, per), np.uint8)
    body[:n, :4 + 4 * maxM0] = np.array(l0, dtype=np.uint32).view(np.uint8)
    body[:n, 4 + 4 * maxM0:per - 8] = x.view(np.uint8)
    body[:n, per - 8:] = labels.reshape(n, 1).view(np.uint8)
    tail = []
    for i in range(cap_out):
        nl = levels[i] if i < n else 0
        tail.append(struct.pack("<I", (4 * maxM + 4) * nl))
        if nl:
            tail.append(np.array(up[i], dtype=np.uint32).tobytes())
    return np.frombuffer(head + body.tobytes() + b"".join(tail), dtype=np.uint8), cnt
