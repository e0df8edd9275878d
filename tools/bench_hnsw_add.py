#!/usr/bin/env python3
"""cvtmi_hnsw_add against cvtmi_hnsw_build on one box: rows added to a graph of BASE x 128-d rows (the config-5 generator, IP,
M = 16, ef_construction = 200, default schedule) in calls of 1, 1 000 and 10 000 rows, the one-shot build of BASE + 10 000 rows, and
recall@10 at ef = 64 of the grown graph next to the one-shot build's.  Every timed add starts from a fresh handle loaded from the
base graph's file (level stream put at BASE draws, as a build leaves it), so the calls do not see each other's rows.  Times are
device events around calls that return when the graph is complete, with the host clock beside them; each figure is the median of
REPEATS runs with the extremes.  Writes profiles/hnsw_add.txt (OUT=... to change)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import cvt_amd
from tools.bench_hnsw_build import recall, rows, truth

BASE = int(os.environ.get("BASE", 100_000))
REPEATS = int(os.environ.get("REPEATS", 3))
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "hnsw_add.txt"))
METRIC, M, EFC, D = 0, 16, 200, 128
lines = []


def log(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    """(device ms, host ms, result) of fn(), which returns with its device work complete"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out


def spread(v):
    v = sorted(v)
    return "%.1f ms (%.1f .. %.1f)" % (v[len(v) // 2], v[0], v[-1])


def main():
    assert torch.cuda.is_available()
    x, q = rows(BASE + 10_000)
    xd = torch.from_numpy(x).cuda()
    log("# tools/bench_hnsw_add.py -- %d + 10000 x %d-d, IP, M=%d efc=%d, default schedule, %d runs each" % (BASE, D, M, EFC, REPEATS))
    cvt_amd.hnsw_build(xd[:20000].contiguous(), METRIC, M, EFC)      # warm-up: module load, first allocations
    base = cvt_amd.hnsw_build(xd[:BASE].contiguous(), METRIC, M, EFC)
    blob = base.save()

    def fresh():
        idx = cvt_amd.HnswIndex(blob, METRIC, D)
        idx.set_level_draws(BASE)
        return idx

    warm = fresh()
    warm.add(xd[BASE:BASE + 2000].contiguous())                      # warm-up of the add path at this shape
    del warm
    full_ms = []
    for _ in range(REPEATS):
        dev, host, full = timed(lambda: cvt_amd.hnsw_build(xd, METRIC, M, EFC))
        full_ms.append(dev)
    n = BASE + 10_000
    med = sorted(full_ms)[len(full_ms) // 2]
    log("build of %d rows: %s  = %.0f rows/s" % (n, spread(full_ms), n / med * 1e3))
    grown = None
    for m in (1, 1000, 10_000):
        ms, hs = [], []
        for _ in range(REPEATS):
            idx = fresh()
            part = xd[BASE:BASE + m].contiguous()
            dev, host, _ = timed(lambda: idx.add(part))
            ms.append(dev); hs.append(host)
            info = idx.last_add()
            if m == 10_000:
                grown = idx
        med = sorted(ms)[len(ms) // 2]
        log("add of %5d rows to %d: %s  host clock %s  = %.0f rows/s  (%d batches, largest %d)" % (
            m, BASE, spread(ms), spread(hs), m / med * 1e3, info[1], info[2]))
    same = grown.save() == full.save()
    log("build(%d) + add(10000) is byte-identical to build(%d): %s (%d is %sa batch boundary of the longer build)" % (
        BASE, n, same, BASE, "" if same else "not necessarily "))
    t = truth(x, q, METRIC)
    rg, rf = recall(grown, q, t, 64), recall(full, q, t, 64)
    log("recall@1 / @10 at ef=64 over %d rows: grown graph %.4f / %.4f   one-shot build %.4f / %.4f" % (n, rg[0], rg[1], rf[0], rf[1]))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
