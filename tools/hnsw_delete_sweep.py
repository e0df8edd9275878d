#!/usr/bin/env python3
"""Deleted nodes of an HNSW graph (cvtmi_hnsw_mark_deleted) measured on the graph of tools/hnsw_masked_sweep.py: 100 K x
128-d clustered unit rows, inner product, M = 32, efConstruction = 80, built on the GPU; 10 000 queries on device pointers, k = 10.

  1. searches with no deleted node, this tree's library against another build of it (--parent-lib: the parent commit's), alternating
     in child processes P B P B ... (--pairs of them); the spread of the P lines is the parent-against-parent spread of the run;
  2. queries/s and recall@10 (against cvtmi_flat_search_masked over the live rows) with 1 % / 10 % / 50 % of the nodes deleted, next to
     cvtmi_hnsw_search_masked on an untouched twin under the mask "not deleted" -- the same kernel, so the figures should coincide;
  3. cvtmi_hnsw_add of 10 000 rows to the 100 K graph with 0 % / 10 % / 50 % of it deleted (a fresh handle per run, loaded from the
     graph's file), the 0 % figure also under --parent-lib.

Wall time of one call between two device synchronisations after warm-up calls, median (and minimum) of the repeats.

    python tools/hnsw_delete_sweep.py [--parent-lib PATH] [--out profiles/hnsw_delete_sweep.txt]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hnsw_delete_sweep.txt"))
ap.add_argument("--parent-lib", default=None, help="libcvtmi.so of the commit to compare with (parts 1 and 3)")
ap.add_argument("--rows", type=int, default=100000)
ap.add_argument("--nq", type=int, default=10000)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--pairs", type=int, default=3, help="parent / branch process pairs of part 1")
ap.add_argument("--child", default=None, help="internal: search | add, one line on stdout")
args = ap.parse_args()
n, D, nq, k, M, efc, ADD = args.rows, 128, args.nq, 10, 32, 80, 10000


def data():
    rng = np.random.default_rng(5)
    cen = rng.normal(size=(1000, D)).astype(np.float32)
    x = cen[rng.integers(0, 1000, n + ADD)] + 0.6 * rng.normal(size=(n + ADD, D)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = x[rng.integers(0, n, nq)] + 0.15 * rng.normal(size=(nq, D)).astype(np.float32)
    return x, (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def timed(torch, fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(min(ms))


def child():
    import torch
    import cvt_amd
    x, q = data()
    xd, qd = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
    ix = cvt_amd.hnsw_build(xd[:n].contiguous(), 0, M, efc)
    if args.child == "search":
        cells = []
        for kk, ef in ((5, 1000), (5, 200), (10, 64)):
            med, lo = timed(torch, lambda: ix.search(qd, kk, ef), args.reps)
            cells.append("k=%d ef=%d %.0f q/s (median %.2f ms, min %.2f)" % (kk, ef, nq / med * 1e3, med, lo))
        print(" | ".join(cells), flush=True)
        return
    blob = ix.save()
    part = xd[n:].contiguous()
    ms = []
    for r in range(args.reps + 1):          # (the first run warms the add path up and is dropped)
        idx = cvt_amd.HnswIndex(blob, 0, D)
        idx.set_level_draws(n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx.add(part)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        idx.close()
    ms = sorted(ms[1:])
    print("add of %d rows to %d, none deleted: median %.1f ms (%.1f .. %.1f)" % (ADD, n, ms[len(ms) // 2], ms[0], ms[-1]), flush=True)


def recall(got, truth):
    hit = (got.unsqueeze(2) == truth.unsqueeze(1)) & (truth.unsqueeze(1) >= 0)
    want = (truth >= 0).sum(dim=1).clamp(min=1)
    return float((hit.any(dim=1).sum(dim=1).float() / want.float()).mean())


def main():
    import torch
    import cvt_amd
    assert torch.cuda.is_available(), "the sweep measures on the GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def run_child(what, lib):
        env = dict(os.environ)
        if lib:
            env["CVTMI_LIB"] = lib
        else:
            env.pop("CVTMI_LIB", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--rows", str(n), "--nq", str(nq), "--reps", str(args.reps)],
                           env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("child %s failed (%d): %s" % (what, r.returncode, (r.stdout + r.stderr)[-2000:]))
        return r.stdout.strip().splitlines()[-1]

    say("# hnsw_delete_sweep: %d x %d-d rows, IP, M = %d, efC = %d (cvtmi_hnsw_build_dev, default schedule), %d queries, k = %d; device %s" % (
        n, D, M, efc, nq, k, torch.cuda.get_device_name(0)))
    # ---- 1. no deleted node: the two libraries, alternating
    say("# 1. searches with no deleted node, one process per line, %d calls after 2 warm-up calls" % args.reps)
    if args.parent_lib:
        for _ in range(args.pairs):
            say("parent | " + run_child("search", args.parent_lib))
            say("branch | " + run_child("search", None))
    else:
        say("(no --parent-lib: not measured)")
    # ---- 2. deleted nodes against the mask "not deleted"
    x, q = data()
    xd, qd = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
    ix = cvt_amd.hnsw_build(xd[:n].contiguous(), 0, M, efc)
    blob = ix.save()
    twin = cvt_amd.HnswIndex(blob, 0, D)
    flat = cvt_amd.FlatIndex(0, D)
    flat.add(xd[:n].contiguous())
    gen = torch.Generator().manual_seed(7)
    say("# 2. deleted nodes: search() on the marked handle | search_masked() on an untouched twin under the mask of the live nodes; recall@10 against cvtmi_flat_search_masked over the live rows; median of 3")
    say("%5s %7s %8s | %10s %11s %9s | %10s %11s %9s | %7s" % ("ef", "deleted", "live", "ms", "queries/s", "recall@10", "masked ms", "queries/s", "recall@10", "slots"))
    ids = torch.arange(n, dtype=torch.int64)
    for frac in (0.01, 0.1, 0.5):
        dead = torch.rand(n, generator=gen) < frac
        live_words = ix._mask_words((~dead).cuda(), True)
        truth = flat.search_masked(qd, k, live_words)[1]
        ix.unmark_deleted(ids.cuda())
        changed = ix.mark_deleted(ids[dead].cuda())
        assert changed == int(dead.sum()) == ix.deleted_count()
        for ef in (64, 1000):
            med, _ = timed(torch, lambda: ix.search(qd, k, ef), 3, warm=1)
            slots = ix.last_masked()[0]
            r1 = recall(ix.search(qd, k, ef)[1], truth)
            med2, _ = timed(torch, lambda: twin.search_masked(qd, k, ef, live_words), 3, warm=1)
            r2 = recall(twin.search_masked(qd, k, ef, live_words)[1], truth)
            say("%5d %6.0f%% %8d | %10.1f %11.0f %9.4f | %10.1f %11.0f %9.4f | %7d" % (
                ef, frac * 100, n - changed, med, nq / med * 1e3, r1, med2, nq / med2 * 1e3, r2, slots))
    ix.unmark_deleted(ids.cuda())
    # ---- 3. add on a graph with deleted nodes
    say("# 3. cvtmi_hnsw_add of %d rows to the %d-row graph (fresh handle per run, level stream continued), default schedule, %d runs after one warm-up run" % (ADD, n, args.reps))
    if args.parent_lib:
        say("parent | " + run_child("add", args.parent_lib))
    say("branch | " + run_child("add", None))
    part = xd[n:].contiguous()
    for frac in (0.1, 0.5):
        dead = torch.rand(n, generator=gen) < frac
        ms = []
        for r in range(args.reps + 1):
            idx = cvt_amd.HnswIndex(blob, 0, D)
            idx.set_level_draws(n)
            idx.mark_deleted(ids[dead].cuda())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            idx.add(part)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            info = idx.last_add()
            if r == args.reps:
                live_words = idx._mask_words(torch.cat([~dead, torch.ones(ADD, dtype=torch.bool)]).cuda(), True)
                full = cvt_amd.FlatIndex(0, D)
                full.add(xd)
                rec = recall(idx.search(qd, k, 64)[1], full.search_masked(qd, k, live_words)[1])
                full.close()
            idx.close()
        ms = sorted(ms[1:])
        say("branch | add of %d rows to %d, %.0f %% deleted: median %.1f ms (%.1f .. %.1f), %d batches, largest %d; recall@10 at ef = 64 afterwards %.4f" % (
            ADD, n, frac * 100, ms[len(ms) // 2], ms[0], ms[-1], info[1], info[2], rec))
    twin.close()
    flat.close()
    ix.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    child() if args.child else main()
