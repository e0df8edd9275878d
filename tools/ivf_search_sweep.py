#!/usr/bin/env python3
"""Row-level IVF search (cvtmi_opq_search_ivf) over batch size, lists probed and k, next to its two yardsticks, on one handle and in
one process: 1 M x 128-d rows, M = 16, 1024 and 8192 coarse lists.

Per cell, device time by HIP events on the call's stream (median of the repeats after two warm-up calls):
  (a) cvtmi_opq_search_ivf_dev
  (b) cvtmi_opq_query_video_dev, same queries and nprobe: the same probing, tables and look-ups without the selection
      (one video per 256 entries; its time includes filling the nq x videos score matrix)
  (c) cvtmi_opq_search_dev over the same rows in a coarseK = 1 index (the exhaustive scan; it does not depend on nprobe)
  (d) recall@k of (a) against the same kernel probing 128 lists, the most the entry takes (first 64 queries)

    python tools/ivf_search_sweep.py [--out profiles/ivf_search_sweep.txt] [--rows 1000000] [--quick]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import cvt_amd
from cvt_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_search_sweep.txt"))
ap.add_argument("--rows", type=int, default=1000000)
ap.add_argument("--quick", action="store_true", help="a corner of the grid (rehearsal)")
args = ap.parse_args()
assert torch.cuda.is_available(), "the sweep measures on the GPU"
dev = torch.device("cuda", 0)
D, M, K, n = 128, 16, 256, args.rows
NQ = (1, 64) if args.quick else (1, 64, 1000, 10000)
NPROBE = (1, 16) if args.quick else (1, 3, 16, 64)
KS = (10, 100) if args.quick else (10, 100, 1000)
LISTS = (1024,) if args.quick else (1024, 8192)
TRUTH_NPROBE, TRUTH_NQ = 128, 64
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


def clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30)
        return "; ".join(l.strip() for l in r.stdout.splitlines() if "sclk" in l or "mclk" in l)[:300]
    except Exception as e:   # noqa: BLE001
        return "not read (%s)" % type(e).__name__


say("# ivf_search_sweep: %d x %d-d rows (synth.sift_like), M = %d, K = %d; device %s" % (n, D, M, K, torch.cuda.get_device_name(0)))
say("# clocks before: %s" % clocks())
x = synth.sift_like(n, D, device="cuda")
qall = synth.sift_like(max(NQ), D, seed=0xBEEF, device="cuda")
gen = torch.Generator().manual_seed(5)

# (c): the exhaustive scan over the same rows, coarseK = 1
books1 = synth.train_books(x[:65536], M, K, iters=2)
flat = cvt_amd.OpqIndex(np.zeros((1, D), np.float32), books1)
_, c1 = flat.encode(x)
flat.add_codes(c1)
exh = {}
for nq in NQ:
    for k in KS:
        q = qall[:nq]
        exh[(nq, k)] = timed(lambda: flat.search(q, k, rotate=False), nq)
flat.close()
del c1

say("%8s %6s %6s %5s | %10s %10s %10s | %7s %7s | %9s  %s" % ("coarseK", "nq", "nprobe", "k", "(a) ivf ms", "(b) vid ms", "(c) exh ms", "a/b", "c/a",
                                                                  "recall@k", "grid of (a)"))
for L in LISTS:
    sel = torch.randperm(n, generator=gen)[:L].to(dev)
    coarse = x[sel]
    pick = torch.randint(0, L, (65536,), generator=gen).to(dev)
    books = synth.train_books(x[:65536] - coarse[pick], M, K, iters=2)   # codebooks of residual-like rows
    ix = cvt_amd.OpqIndex(coarse.cpu().numpy(), books)
    lists, codes = ix.encode(x)
    videos = (torch.arange(n, device=dev, dtype=torch.int32) // 256).contiguous()
    n_videos = (n + 255) // 256
    ix.add_codes(codes, lists, videos)
    cnt = torch.bincount(lists[lists >= 0].long(), minlength=L)
    say("# coarseK = %d: longest list %d rows, mean %.1f, empty lists %d, videos %d" % (L, int(cnt.max()), float(cnt.float().mean()), int((cnt == 0).sum()),
                                                                                     n_videos))
    for nq in NQ:
        q = qall[:nq]
        qt = qall[:min(nq, TRUTH_NQ)]
        for k in KS:
            _, truth = ix.search_ivf(qt, TRUTH_NPROBE, k, rotate=False)
            truth = truth.cpu().numpy()
            for nprobe in NPROBE:
                a = timed(lambda: ix.search_ivf(q, nprobe, k, rotate=False), nq)
                p = ix.last_ivf_plan()
                b = timed(lambda: ix.query_video(q, nprobe, n_videos, rotate=False), nq)
                _, got = ix.search_ivf(qt, nprobe, k, rotate=False)
                got = got.cpu().numpy()
                hit = sum(len(set(g[g >= 0].tolist()) & set(t[t >= 0].tolist())) for g, t in zip(got, truth))
                tot = sum(int((t >= 0).sum()) for t in truth)
                c = exh[(nq, k)]
                say("%8d %6d %6d %5d | %10.3f %10.3f %10.3f | %7.2f %7.2f | %9.4f  rule %d G=%d groups=%d pieces=%d" % (
                    L, nq, nprobe, k, a, b, c, a / b, c / a, hit / max(tot, 1), p["rule"], p["G"], p["groups"], p["pieces"]))
    ix.close()
say("# clocks after: %s" % clocks())
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
