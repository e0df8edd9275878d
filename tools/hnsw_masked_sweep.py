#!/usr/bin/env python3
"""Masked HNSW search (cvtmi_hnsw_search_masked) next to the unmasked one, on one graph and in one process: 100 K x 128-d rows
(bench_hnsw.py's clustered unit rows, inner product), M = 32, efConstruction = 80, built on the GPU; 10 000 queries, k = 10,
ef in {64, 1000}; random masks of density 1.0 / 0.5 / 0.1 / 0.01.

Per cell: wall time of one call on device pointers between two device synchronisations, after a warm-up call (median of the
repeats) -> queries/s; the slots and scratch bytes the masked plan took (cvtmi_hnsw_last_masked); recall@10 against
cvtmi_flat_search_masked over the same rows and the same mask (the exact filtered answer), and against cvtmi_flat_search for the
unmasked row.

    python tools/hnsw_masked_sweep.py [--out profiles/hnsw_masked_sweep.txt] [--rows 100000] [--nq 10000] [--reps 3]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import cvt_amd

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hnsw_masked_sweep.txt"))
ap.add_argument("--rows", type=int, default=100000)
ap.add_argument("--nq", type=int, default=10000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--append", action="store_true", help="add to the file instead of replacing it (a second graph size)")
args = ap.parse_args()
assert torch.cuda.is_available(), "the sweep measures on the GPU"
n, D, nq, k, M, efc = args.rows, 128, args.nq, 10, 32, 80
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def recall(got, truth):
    """mean share of the true (non-padding) labels of a query found among its results"""
    hit = (got.unsqueeze(2) == truth.unsqueeze(1)) & (truth.unsqueeze(1) >= 0)
    want = (truth >= 0).sum(dim=1).clamp(min=1)
    return float((hit.any(dim=1).sum(dim=1).float() / want.float()).mean())


rng = np.random.default_rng(5)
cen = rng.normal(size=(1000, D)).astype(np.float32)
x = cen[rng.integers(0, 1000, n)] + 0.6 * rng.normal(size=(n, D)).astype(np.float32)
x /= np.linalg.norm(x, axis=1, keepdims=True)
q = x[rng.integers(0, n, nq)] + 0.15 * rng.normal(size=(nq, D)).astype(np.float32)
q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
xd, qd = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
say("# hnsw_masked_sweep: %d x %d-d rows, IP, M = %d, efC = %d (cvtmi_hnsw_build_dev, default schedule), %d queries, k = %d; device %s" % (
    n, D, M, efc, nq, k, torch.cuda.get_device_name(0)))
t0 = time.perf_counter()
ix = cvt_amd.hnsw_build(xd, 0, M, efc)
torch.cuda.synchronize()
say("# build: %.1f s" % (time.perf_counter() - t0))
flat = cvt_amd.FlatIndex(0, D)
flat.add(xd)
gen = torch.Generator().manual_seed(7)
masks = {}
for dens in (1.0, 0.5, 0.1, 0.01):
    allowed = torch.rand(n, generator=gen) < dens if dens < 1.0 else torch.ones(n, dtype=torch.bool)
    masks[dens] = (ix._mask_words(allowed.cuda(), True), int(allowed.sum()))
truth_all = flat.search(qd, k)[1]
truth = {dens: flat.search_masked(qd, k, w)[1] for dens, (w, _) in masks.items()}
torch.cuda.synchronize()
say("%5s %9s %9s | %10s %11s | %7s %13s | %9s" % ("ef", "mask", "allowed", "ms", "queries/s", "slots", "scratch bytes", "recall@10"))
for ef in (64, 1000):
    ms = timed(lambda: ix.search(qd, k, ef))
    say("%5d %9s %9d | %10.1f %11.0f | %7s %13s | %9.4f" % (ef, "unmasked", n, ms, nq / ms * 1e3, "-", "-", recall(ix.search(qd, k, ef)[1], truth_all)))
    for dens, (w, cnt) in masks.items():
        ms = timed(lambda: ix.search_masked(qd, k, ef, w))
        slots, cap, scratch, form = ix.last_masked()
        say("%5d %9.2f %9d | %10.1f %11.0f | %7d %13d | %9.4f" % (ef, dens, cnt, ms, nq / ms * 1e3, slots, scratch, recall(ix.search_masked(qd, k, ef, w)[1], truth[dens])))
ix.close()
flat.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a" if args.append else "w") as f:
    f.write("\n".join(lines) + "\n")
