#!/usr/bin/env python3
"""cvtmi_flat_remove_labels against the best a caller could do without it, in one process.

  (a) remove_labels of a random 1 % and of a random 50 % of the rows (the set is a device tensor: the _dev entry);
  (b) cvtmi_flat_reset + cvtmi_flat_add_dev of a device-resident copy of the kept rows and labels -- which costs a second copy of
      the table in HBM that (a) never needs.
Both are timed by a host clock around work that ends in a device synchronise, alternating, after a warm-up of each; the index is put
back (reset + add of the full table, not timed) before every (a).  Median, min and max of REPS repeats; the bytes the move of (a)
needs by the algorithm (every row behind the first dropped one: source -> chunk scratch -> destination, with its label and norm;
fp32: one more read of the kept rows for the score bias) over the median time.  The answers of (a) and (b) are compared.
Once per shape, for context: what the host mirror paid per removePoint before -- rows sorted on the host and uploaded again.

  ROWS_F32 / ROWS_U8 / D / REPS in the environment change the shapes (default 1 M x 128-d fp32, 10 M x 128-d uint8, 7 repeats);
  CHUNK_MB=0,16,256 repeats everything per "remove_chunk" (given as MB of rows; 0 = the library's default)."""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import cvt_amd
from cvt_amd import capi

dev = torch.device("cuda", 0)
D = int(os.environ.get("D", 128))
REPS = int(os.environ.get("REPS", 7))
CHUNK_MB = [int(v) for v in os.environ.get("CHUNK_MB", "0").split(",")]
SHAPES = [("fp32 L2", 1, int(os.environ.get("ROWS_F32", 1_000_000))), ("uint8 L2", 2, int(os.environ.get("ROWS_U8", 10_000_000)))]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return "median %8.3f ms  (min %8.3f, max %8.3f, %d runs)" % (statistics.median(ts), min(ts), max(ts), len(ts))


def main():
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    for name, metric, n in SHAPES:
        if n <= 0:
            continue
        rb = D if metric == 2 else 4 * D
        per_row = rb + 8 + (4 if metric == 2 and D % 32 == 0 and D <= 512 else 0)
        x = torch.randint(0, 256, (n, D), generator=g, device=dev, dtype=torch.uint8) if metric == 2 else torch.randn((n, D), generator=g, device=dev)
        q = x[torch.randint(0, n, (16,), generator=g, device=dev)].contiguous()
        ix, other = cvt_amd.FlatIndex(metric, D), cvt_amd.FlatIndex(metric, D)
        print("%s  %d x %d-d  (%.2f GB of rows)" % (name, n, D, n * rb / 1e9), flush=True)

        def refill():
            capi._check(capi.lib().cvtmi_flat_reset(ix.h))
            ix.add(x)

        for pct in (1, 50):
            drop = torch.randperm(n, generator=g, device=dev)[:n * pct // 100].contiguous()
            keep = torch.ones(n, dtype=torch.bool, device=dev)
            keep[drop] = False
            kept_rows, kept_labels = x[keep].contiguous(), torch.nonzero(keep).reshape(-1).contiguous()   # (b)'s second copy of the table
            first = int(drop.min())
            moved = int(keep[first:].sum())
            bytes_a = 4 * moved * per_row + (int(keep.sum()) * rb if metric != 2 else 0)

            def a():
                assert ix.remove_labels(drop) == drop.numel()

            def b():
                capi._check(capi.lib().cvtmi_flat_reset(other.h))
                other.add(kept_rows, kept_labels)

            for mb in CHUNK_MB:
                ix.set_param("remove_chunk", (mb << 20) // rb)
                ta, tb = [], []
                for rep in range(REPS + 1):   # the first round warms both up
                    refill()
                    t = timed(a)
                    u = timed(b)
                    if rep:
                        ta.append(t); tb.append(u)
                da, ia = ix.search(q, 10)
                db, ib = other.search(q, 10)
                assert torch.equal(ia, ib) and torch.equal(da, db), "the two ways disagree"
                ma = statistics.median(ta)
                print("  drop %2d %%  chunk %s" % (pct, "%d MB" % mb if mb else "default"))
                print("             (a) remove_labels           %s   %.0f GB/s over %.2f GB the move needs" % (stats(ta), bytes_a / ma / 1e6, bytes_a / 1e9))
                print("             (b) reset + add_dev of kept  %s   (a) / (b) = %.2f" % (stats(tb), ma / statistics.median(tb)), flush=True)
            del kept_rows, kept_labels, keep, drop
        # context: the rebuild the host mirror ran for one removePoint -- sort by label on the host, upload everything
        host = x.cpu().numpy()
        labels = np.arange(n, dtype=np.int64)
        t0 = time.perf_counter()
        order = np.argsort(labels, kind="stable")
        rows = host[order]
        capi._check(capi.lib().cvtmi_flat_reset(other.h))
        other.add(rows, labels[order])
        torch.cuda.synchronize()
        print("  context: host sort + re-upload of all rows (one run)  %.1f ms" % ((time.perf_counter() - t0) * 1e3), flush=True)
        ix.close(); other.close()
        del x, host, rows


if __name__ == "__main__":
    main()
