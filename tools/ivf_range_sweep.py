#!/usr/bin/env python3
"""Range search over the probed lists (cvtmi_opq_range_search_ivf) over batch size, lists probed and result size, next to its
yardstick, on one handle and in one process: 1 M x 128-d rows, M = 16, 8192 and 1024 coarse lists.

Per cell, device time by HIP events on the call's stream (median of the repeats after two warm-up calls), ROUNDS times, the two
calls alternating:
  (y) cvtmi_opq_search_ivf_dev, k = 100, same handle, queries and nprobe: the same probing and tables, a top-k selection per row
  (r) cvtmi_opq_range_search_ivf_dev into arrays that hold the result (one call: scan, offsets, fill, rescan), at two radii -- the
      median over 64 sample queries of the 100-th and of the 5000-th smallest score among the entries they probe (where the
      probed lists hold fewer: of nine tenths of them); the median hit count of the batch is printed
      with "ivf_range_spill" at its default and at 0 (every part with a hit is walked twice: the price of a second table build)
The yardstick's spread is the range of its ROUNDS medians.  Every cell also checks that the results of both spill settings equal
those of spill = 2^30 (no part walked twice while the area fits).

    python tools/ivf_range_sweep.py [--out profiles/ivf_range_sweep.txt] [--rows 1000000] [--quick]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import cvt_amd
from cvt_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_range_sweep.txt"))
ap.add_argument("--rows", type=int, default=1000000)
ap.add_argument("--quick", action="store_true", help="a corner of the grid (rehearsal)")
args = ap.parse_args()
assert torch.cuda.is_available(), "the sweep measures on the GPU"
dev = torch.device("cuda", 0)
D, M, K, n = 128, 16, 256, args.rows
NQ = (1, 64) if args.quick else (1, 64, 1000, 10000)
NPROBE = (3, 16)
LISTS = (1024,) if args.quick else (8192, 1024)
TARGETS = (100, 5000)
ROUNDS, SAMPLE, SPILL_DEFAULT = 3, 64, 4096
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, nq):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    reps = 5 if nq >= 1000 else 15
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def radius_for(ix, q, nprobe, target):
    """the median over the sample queries of their T-th smallest probed score, T = min(target, 0.9 x entries probed)"""
    lims, d, _ = ix.range_search_ivf(q, nprobe, float("inf"), rotate=False)
    lims, d = lims.cpu().numpy(), d.cpu().numpy()
    cut = []
    for f in range(q.shape[0]):
        s = np.sort(d[lims[f]:lims[f + 1]])
        if s.size:
            cut.append(s[min(target, int(0.9 * s.size))])
    return float(np.median(cut))


say("# ivf_range_sweep: %d x %d-d rows (synth.sift_like), M = %d, K = %d; device %s" % (n, D, M, K, torch.cuda.get_device_name(0)))
x = synth.sift_like(n, D, device="cuda")
qall = synth.sift_like(max(NQ), D, seed=0xBEEF, device="cuda")
gen = torch.Generator().manual_seed(5)
say("%8s %6s %6s %7s | %9s %9s | %9s %9s %9s | %7s %7s | %5s  %s" % ("coarseK", "nq", "nprobe", "hits", "(y) ms", "y spread", "(r) ms", "r spread",
                                                                        "spill0 ms", "r/y", "s0/r", "equal", "grid of (r)"))
for L in LISTS:
    sel = torch.randperm(n, generator=gen)[:L].to(dev)
    coarse = x[sel]
    pick = torch.randint(0, L, (65536,), generator=gen).to(dev)
    books = synth.train_books(x[:65536] - coarse[pick], M, K, iters=2)   # codebooks of residual-like rows
    ix = cvt_amd.OpqIndex(coarse.cpu().numpy(), books)
    lists, codes = ix.encode(x)
    ix.add_codes(codes, lists)
    cnt = torch.bincount(lists[lists >= 0].long(), minlength=L)
    say("# coarseK = %d: longest list %d rows, mean %.1f, empty lists %d" % (L, int(cnt.max()), float(cnt.float().mean()), int((cnt == 0).sum())))
    for nprobe in NPROBE:
        radii = [radius_for(ix, qall[:SAMPLE], nprobe, t) for t in TARGETS]
        for nq in NQ:
            q = qall[:nq]
            for radius in radii:
                cvt_amd.set_tuning("ivf_range_spill", 1 << 30)
                ref = ix.range_search_ivf(q, nprobe, radius, rotate=False)
                total = int(ref[0][-1])
                hits = float(np.median(np.diff(ref[0].cpu().numpy())))
                out = (torch.empty_like(ref[0]), torch.empty(max(total, 1), dtype=torch.float32, device=dev),
                       torch.empty(max(total, 1), dtype=torch.int64, device=dev))
                yk = (torch.empty((nq, 100), dtype=torch.float32, device=dev), torch.empty((nq, 100), dtype=torch.int64, device=dev))
                y, r, s0, equal = [], [], [], True
                for _ in range(ROUNDS):
                    y.append(timed(lambda: ix.search_ivf(q, nprobe, 100, rotate=False, out=yk), nq))
                    for spill, acc in ((SPILL_DEFAULT, r), (0, s0)):
                        cvt_amd.set_tuning("ivf_range_spill", spill)
                        acc.append(timed(lambda: ix.range_search_ivf(q, nprobe, radius, rotate=False, out=out), nq))
                        if spill:
                            p = ix.last_range_plan()
                        torch.cuda.synchronize()
                        equal = equal and torch.equal(out[0], ref[0]) and torch.equal(out[1][:total].view(torch.int32), ref[1].view(torch.int32)) \
                            and torch.equal(out[2][:total], ref[2])
                ym, rm, sm = float(np.median(y)), float(np.median(r)), float(np.median(s0))
                say("%8d %6d %6d %7.0f | %9.3f %9.3f | %9.3f %9.3f %9.3f | %7.2f %7.2f | %5s  rule %d G=%d groups=%d pieces=%d spill=%d" % (
                    L, nq, nprobe, hits, ym, max(y) - min(y), rm, max(r) - min(r), sm, rm / ym, sm / rm, "yes" if equal else "NO",
                    p["rule"], p["G"], p["groups"], p["pieces"], p["spill"]))
    ix.close()
cvt_amd.set_tuning("ivf_range_spill", SPILL_DEFAULT)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
