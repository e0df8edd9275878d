#!/usr/bin/env python3
"""cvtmi_flat_rerank_dev from its three row sources, against the exhaustive search of the same handle, in one process.

  k = 100, nq = 1000 queries, R uniformly random candidate rows per query (all valid; a row drawn twice counts once):
    (a) 1 M x 128-d fp32 L2, blocked rows           ("rerank_rows_copy" 0, before anything has built the row-major copy)
    (b) the same table, the row-major copy          ("rerank_rows_copy" 1)
    (c) 10 M x 128-byte uint8 L2                    (row-major as it is)
  and cvtmi_flat_search_dev(k = 100) for the same queries on the same handle: from which R onward the exhaustive search is the
  better call.
Timing: device events around CALLS calls on one stream, after a warm-up of every shape; median, min and max of REPS repeats, per
call.  MEASURED: the times.  MODELLED: the bytes -- distinct valid candidates x row bytes, times 8 for the blocked rows (16 useful
bytes of every 128-byte line) -- and hence the bytes per second printed beside them.

  ROWS_F32 / ROWS_U8 / NQ / RS / K / REPS / CALLS in the environment change the shapes."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import cvt_amd

dev = torch.device("cuda", 0)
REPS = int(os.environ.get("REPS", 9))
CALLS = int(os.environ.get("CALLS", 100))
NQ = int(os.environ.get("NQ", 1000))
K = int(os.environ.get("K", 100))
RS = [int(v) for v in os.environ.get("RS", "100,1000").split(",")]
SHAPES = [("fp32 L2", 1, int(os.environ.get("ROWS_F32", 1_000_000)), 128), ("uint8 L2", 2, int(os.environ.get("ROWS_U8", 10_000_000)), 128)]
SOURCE = {0: "row-major primary rows", 1: "blocked rows", 2: "row-major copy"}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / CALLS


def series(fn):
    for _ in range(2):
        timed(fn)
    return [timed(fn) for _ in range(REPS)]


def stats(ts):
    return "median %8.3f ms  (min %8.3f, max %8.3f, %d x %d calls)" % (statistics.median(ts), min(ts), max(ts), len(ts), CALLS)


def main():
    assert torch.cuda.is_available(), "needs the GPU: there is no fallback"
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    for name, metric, n, D in SHAPES:
        if n <= 0:
            continue
        rb = D if metric == 2 else 4 * D
        if metric == 2:
            x = torch.randint(0, 256, (n, D), generator=g, device=dev, dtype=torch.uint8)
            q = torch.randint(0, 256, (NQ, D), generator=g, device=dev, dtype=torch.uint8)
        else:
            x = torch.randn((n, D), generator=g, device=dev)
            q = torch.randn((NQ, D), generator=g, device=dev)
        ix = cvt_amd.FlatIndex(metric, D)
        ix.add(x)
        del x
        torch.cuda.empty_cache()
        print("%s  %d x %d-d  (%.2f GB of rows), nq = %d, k = %d" % (name, n, D, n * rb / 1e9, NQ, K), flush=True)
        cands = {}
        for R in RS:
            c = torch.randint(0, n, (NQ, R), generator=g, device=dev, dtype=torch.int64)
            s, _ = torch.sort(c, dim=1)
            distinct = int((s[:, 1:] != s[:, :-1]).sum()) + NQ
            cands[R] = (c, distinct)
        for copy in ((0, 1) if metric != 2 else (0,)):
            ix.set_param("rerank_rows_copy", copy)
            for R in RS:
                c, distinct = cands[R]
                ts = series(lambda: ix.rerank(q, c, K))
                src, lanes, groups, lds = ix.last_rerank()
                model = distinct * rb * (8 if src == 1 else 1)
                med = statistics.median(ts)
                print("  rerank R = %-5d %-22s %s" % (R, SOURCE[src], stats(ts)))
                print("      lanes %d, %d workgroups, %d bytes of LDS each; %d distinct valid candidates; modelled %.3f GB per call, %.2f TB/s over the median"
                      % (lanes, groups, lds, distinct, model / 1e9, model / 1e12 / (med / 1e3)), flush=True)
        ts = series(lambda: ix.search(q, K))
        print("  exhaustive cvtmi_flat_search, k = %d       %s   (answered by route %d)" % (K, stats(ts), ix.last_search()[0]), flush=True)
        ix.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
