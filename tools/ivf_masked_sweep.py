#!/usr/bin/env python3
"""Masked IVF search (cvtmi_opq_search_ivf_masked) next to the unmasked one, on one handle and in one process: 1 M x 128-d rows,
M = 16, 8192 coarse lists, k = 100, nq in {1, 64, 10000} x nprobe in {3, 16}.

Per cell, device time by HIP events on the call's stream (median of the repeats after two warm-up calls):
  (a)     cvtmi_opq_search_ivf_dev, unmasked
  (c)     cvtmi_opq_search_ivf_masked_dev with an all-ones mask: (a) plus the launch that orders the mask and one bit per row
  (d10)   ... with 10 % of the entries allowed at random
  (d1)    ... with 1 % allowed at random
  (e)     ... with 1 % allowed as whole videos of 256 consecutive entries (cvtmi_opq_mask_videos)
and the share of (query, list) pairs of the cell that hold an allowed entry at all: the pairs whose table is still built.

--unmasked-only prints column (a) alone and touches no masked entry: with CVTMI_LIB pointing at the library of another commit it is
that commit's (a) on the same data -- run twice, the two runs give the spread (a) has to lie in.

    python tools/ivf_masked_sweep.py [--out profiles/ivf_search_masked.txt] [--rows 1000000] [--unmasked-only] [--tag TEXT]
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_search_masked.txt"))
ap.add_argument("--rows", type=int, default=1000000)
ap.add_argument("--lists", type=int, default=8192)
ap.add_argument("--unmasked-only", action="store_true")
ap.add_argument("--only", default="", help="nq:nprobe of the one cell to run (a profiler run)")
ap.add_argument("--tag", default="this tree")
args = ap.parse_args()
assert torch.cuda.is_available(), "the sweep measures on the GPU"
dev = torch.device("cuda", 0)
D, M, K, n, L, k = 128, 16, 256, args.rows, args.lists, 100
CELLS = [(nq, nprobe) for nq in (1, 64, 10000) for nprobe in (3, 16)]
if args.only:
    CELLS = [tuple(int(t) for t in args.only.split(":"))]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, nq):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    reps = 7 if nq >= 1000 else 21
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


def words_of(allowed):
    """bool [n] on the device -> int64 words (bit i & 63 of word i >> 6)"""
    pad = (-allowed.shape[0]) % 64
    bits = torch.nn.functional.pad(allowed.to(torch.int64), (0, pad)).reshape(-1, 64)
    return (bits << torch.arange(64, device=allowed.device, dtype=torch.int64)).sum(dim=1).contiguous()


say("# ivf_masked_sweep (%s): %d x %d-d rows (synth.sift_like), M = %d, K = %d, %d lists, k = %d; device %s; library %s" % (
    args.tag, n, D, M, K, L, k, torch.cuda.get_device_name(0), os.path.relpath(cvt_amd.capi.LIB_PATH, ROOT)))
say("# clocks before: %s" % clocks())
x = synth.sift_like(n, D, device="cuda")
qall = synth.sift_like(max(c[0] for c in CELLS), D, seed=0xBEEF, device="cuda")
gen = torch.Generator().manual_seed(5)
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
say("# longest list %d rows, mean %.1f, empty lists %d, videos %d" % (int(cnt.max()), float(cnt.float().mean()), int((cnt == 0).sum()), n_videos))

if args.unmasked_only:
    say("%6s %6s | %10s" % ("nq", "nprobe", "(a) ivf ms"))
    for nq, nprobe in CELLS:
        q = qall[:nq]
        say("%6d %6d | %10.3f" % (nq, nprobe, timed(lambda: ix.search_ivf(q, nprobe, k, rotate=False), nq)))
else:
    masks = {}
    masks["c"] = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device=dev)
    masks["d10"] = words_of(torch.rand(n, generator=gen).to(dev) < 0.10)
    masks["d1"] = words_of(torch.rand(n, generator=gen).to(dev) < 0.01)
    vids = torch.randperm(n_videos, generator=gen)[:max(1, n_videos // 100)].to(torch.int32).to(dev)
    masks["e"] = ix.mask_from_videos(vids)
    torch.cuda.synchronize()
    allowed = {}
    for name, w in masks.items():
        b = ((w.unsqueeze(1) >> torch.arange(64, device=dev, dtype=torch.int64)) & 1).reshape(-1)[:n].bool()
        allowed[name] = b
        per_list = torch.bincount(lists[b & (lists >= 0)].long(), minlength=L)
        say("# mask %-3s: %d entries allowed (%.2f %%), %d of %d lists hold one" % (name, int(b.sum()), 100.0 * float(b.sum()) / n, int((per_list > 0).sum()), L))
    say("%6s %6s | %10s %10s %10s %10s %10s | %6s %6s %6s %6s | pairs with an allowed entry: %s  grid" % (
        "nq", "nprobe", "(a) ivf ms", "(c) ones", "(d) 10 %", "(d) 1 %", "(e) 1 % vid", "c/a", "d10/a", "d1/a", "e/a", "d10 / d1 / e"))
    for nq, nprobe in CELLS:
        q = qall[:nq]
        a = timed(lambda: ix.search_ivf(q, nprobe, k, rotate=False), nq)
        t = {}
        for name, w in masks.items():
            t[name] = timed(lambda: ix.search_ivf_masked(q, nprobe, k, w, rotate=False), nq)
        p = ix.last_ivf_masked()
        # the lists a query probes (a statistic: torch's distances, not the library's sequential ones), first 256 queries
        probed = torch.cdist(q[:min(nq, 256)], coarse).topk(nprobe, dim=1, largest=False).indices
        share = {}
        for name in ("d10", "d1", "e"):
            per_list = torch.bincount(lists[allowed[name] & (lists >= 0)].long(), minlength=L) > 0
            share[name] = float(per_list[probed].float().mean())
        say("%6d %6d | %10.3f %10.3f %10.3f %10.3f %10.3f | %6.2f %6.2f %6.2f %6.2f | %.2f / %.2f / %.2f  rule %d G=%d groups=%d pieces=%d" % (
            nq, nprobe, a, t["c"], t["d10"], t["d1"], t["e"], t["c"] / a, t["d10"] / a, t["d1"] / a, t["e"] / a, share["d10"], share["d1"], share["e"],
            p["rule"], p["G"], p["groups"], p["pieces"]))
ix.close()
say("# clocks after: %s" % clocks())
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a" if os.path.exists(args.out) and args.unmasked_only else "w") as f:
    f.write("\n".join(lines) + "\n")
