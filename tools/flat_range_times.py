#!/usr/bin/env python3
"""cvtmi_flat_range_search against the exact top-k search it shares its distance work with, in one process.

  (a) cvtmi_flat_search_dev, k = 10, under cvtmi_set_tuning("flat_variant", 1): the exact kernels only (flat.hip; this code is the
      same as before the range search existed);
  (b) cvtmi_flat_range_search_dev with room for the hits (ONE call: scan, offsets, fill, rescan), at a radius with about 100 hits
      per query: the median over the batch of the 100th smallest distance, taken from a k = 100 search.
Both are timed by a host clock around CALLS calls that end in one device synchronise, alternating (a) and (b), after a warm-up of
each.  Median, min and max of REPS repeats, per call; the row bytes the scan needs by the algorithm (every row once per query group:
n x row bytes x groups) over the median time of (b); the plan of (b) (cvtmi_flat_last_range_plan) and its hit count.

  ROWS_F32 / ROWS_U8 / NQ / REPS / CALLS in the environment change the shapes (default 1 M x 128-d fp32 IP, 10 M x 512-d uint8,
  nq = 1, 8, 96, 7 repeats of 10 calls)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import cvt_amd

dev = torch.device("cuda", 0)
REPS = int(os.environ.get("REPS", 7))
CALLS = int(os.environ.get("CALLS", 10))
NQS = [int(v) for v in os.environ.get("NQ", "1,8,96").split(",")]
SHAPES = [("fp32 IP", 0, int(os.environ.get("ROWS_F32", 1_000_000)), 128), ("uint8 L2", 2, int(os.environ.get("ROWS_U8", 10_000_000)), 512)]
HITS = 100


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / CALLS


def stats(ts):
    return "median %7.3f ms  (min %7.3f, max %7.3f, %d x %d calls)" % (statistics.median(ts), min(ts), max(ts), len(ts), CALLS)


def main():
    assert torch.cuda.is_available(), "needs the GPU: there is no fallback"
    g = torch.Generator(device=dev)
    g.manual_seed(9)
    old = cvt_amd.get_tuning("flat_variant")
    cvt_amd.set_tuning("flat_variant", 1)
    try:
        for name, metric, n, D in SHAPES:
            if n <= 0:
                continue
            rb = D if metric == 2 else 4 * D
            if metric == 2:
                x = torch.randint(0, 256, (n, D), generator=g, device=dev, dtype=torch.uint8)
            else:
                x = torch.randn((n, D), generator=g, device=dev)
                x /= x.norm(dim=1, keepdim=True)
            ix = cvt_amd.FlatIndex(metric, D)
            ix.add(x)
            print("%s  %d x %d-d  (%.2f GB of rows)" % (name, n, D, n * rb / 1e9), flush=True)
            for nq in NQS:
                pick = torch.randint(0, n, (nq,), generator=g, device=dev)
                if metric == 2:
                    q = (x[pick].to(torch.int16) + torch.randint(-40, 41, (nq, D), generator=g, device=dev, dtype=torch.int16)).clamp(0, 255).to(torch.uint8).contiguous()
                else:
                    q = x[pick] + 0.05 * torch.randn((nq, D), generator=g, device=dev)
                    q = (q / q.norm(dim=1, keepdim=True)).contiguous()
                d100, _ = ix.search(q, HITS)
                radius = float(d100[:, HITS - 1].to(torch.float64).median())
                cap = nq * HITS * 64
                lims = torch.empty(nq + 1, dtype=torch.int64, device=dev)
                rd = torch.empty(cap, dtype=torch.int32 if metric == 2 else torch.float32, device=dev)
                ri = torch.empty(cap, dtype=torch.int64, device=dev)
                search = lambda: ix.search(q, 10)
                rng = lambda: ix.range_search(q, radius, out=(lims, rd, ri))
                for _ in range(2):
                    timed(search); timed(rng)
                ta, tb = [], []
                for _ in range(REPS):
                    ta.append(timed(search)); tb.append(timed(rng))
                total = int(lims[-1])
                assert total <= cap, (total, cap)
                plan = ix.last_range_plan()
                groups = (nq + plan["qt"] - 1) // plan["qt"]
                ma, mb = statistics.median(ta), statistics.median(tb)
                print("  nq = %-3d radius %.6g: %d hits (%.1f per query)" % (nq, radius, total, total / nq))
                print("    (a) exact search, k = 10   %s" % stats(ta))
                print("    (b) range search           %s   = (a) %+.1f %%" % (stats(tb), (mb / ma - 1) * 100))
                print("        plan %s" % plan)
                print("        rows read by the scan: %.2f GB per call, %.2f TB/s over the median" % (n * rb * groups / 1e9, n * rb * groups / 1e12 / (mb / 1e3)), flush=True)
            ix.close()
            del x
            torch.cuda.empty_cache()
    finally:
        cvt_amd.set_tuning("flat_variant", old)


if __name__ == "__main__":
    main()
