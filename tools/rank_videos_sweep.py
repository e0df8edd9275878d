#!/usr/bin/env python3
"""cvtmi_opq_rank_videos next to the way opq_query gets the same answer without it, on a synthetic index: 8192 coarse lists, M = 16,
two entries per video, 3 lists probed.

Per point (img_num x frames per query video x query videos per call x k), wall-clock time of whole calls from the host, the stream
idle before and after (two warm-up calls -- one where a call takes seconds --, then the median of the repeats; the spread is their range):
  (p) the parent's way, one query video at a time as opq_query's loop runs it: the host entry cvtmi_opq_query_video (the dense
      [frames][img_num] matrix comes down), a numpy fp32 sum one frame at a time, cvtmi_topk_select on the totals
  (h) cvtmi_opq_rank_videos, host pointers, all query videos in one call: only the lists come down
  (d) cvtmi_opq_rank_videos_dev on device tensors, synchronised
Every point also checks that (h) and (d) return the bits of (p).  "PCIe saved" is the score matrix (and the totals that went up
again for the selection) the call no longer moves; "fold GB" what video_frame_sum_kernel reads and writes in the call.

Every point runs in a process of its own under a time limit; the sweep stops at the first that fails.

    python tools/rank_videos_sweep.py [--out profiles/rank_videos_sweep.txt] [--quick]
    python tools/rank_videos_sweep.py --point IMG_NUM,FRAMES,VIDEOS [--reps N] [--device-only]     (one point, printed)
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_videos_sweep.txt"))
ap.add_argument("--quick", action="store_true", help="the small collection only (rehearsal)")
ap.add_argument("--point", default="", help="img_num,frames,videos: measure this point in this process")
ap.add_argument("--reps", type=int, default=0, help="repeats per measurement (0 = by the time one call takes)")
ap.add_argument("--device-only", action="store_true", help="a point without the parent's way (under a profiler)")
args = ap.parse_args()

IMG_NUMS = (100000,) if args.quick else (100000, 1000000)
FRAMES, VIDEOS, KS = (9, 100), (1, 64), (5, 100)
D, M, K, LISTS, NPROBE, PER_VIDEO = 128, 16, 256, 8192, 3, 2
HEADER = "%9s %6s %6s %4s | %10s %10s | %10s %10s | %10s %10s | %7s %7s | %5s | %10s %8s %6s" % (
    "img_num", "frames", "videos", "k", "(p) ms", "p spread", "(h) ms", "h spread", "(d) ms", "d spread", "p/h", "p/d", "equal", "PCIe saved", "fold GB", "chunks")


def timed(fn, sync):
    """median and range in ms of whole calls"""
    sync(); t0 = time.perf_counter(); fn(); sync()
    first = time.perf_counter() - t0
    if first < 1.0:   # (a call of seconds is warm after one)
        fn(); sync()
    reps = args.reps or max(3, min(15, int(3.0 / max(first, 1e-4))))
    ms = []
    for _ in range(reps):
        sync(); t0 = time.perf_counter(); fn(); sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return ms[len(ms) // 2], ms[-1] - ms[0]


def point(img_num, frames, videos):
    import numpy as np
    import torch
    import cvt_amd
    from cvt_amd import synth
    assert torch.cuda.is_available(), "the sweep measures on the GPU"
    dev = torch.device("cuda", 0)
    n = PER_VIDEO * img_num
    x = synth.sift_like(n, D, device="cuda")
    gen = torch.Generator().manual_seed(5)
    coarse = x[torch.randperm(n, generator=gen)[:LISTS].to(dev)]
    pick = torch.randint(0, LISTS, (65536,), generator=gen).to(dev)
    books = synth.train_books(x[:65536] - coarse[pick], M, K, iters=2)   # codebooks of residual-like rows
    ix = cvt_amd.OpqIndex(coarse.cpu().numpy(), books)
    lists, codes = ix.encode(x)
    ix.add_codes(codes, lists, (torch.arange(n, device=dev) % img_num).to(torch.int32))
    nq = frames * videos
    qd = (x[torch.randint(0, n, (nq,), generator=gen).to(dev)] + 0.01 * synth.sift_like(nq, D, seed=0xBEEF, device="cuda")).contiguous()
    qh = qd.cpu().numpy()
    seg = np.arange(videos + 1, dtype=np.int64) * frames
    sync = torch.cuda.synchronize

    def parent(k):
        score = np.empty((videos, k), np.float32); video = np.empty((videos, k), np.int64)
        for s in range(videos):
            ms = ix.query_video(qh[seg[s]:seg[s + 1]], NPROBE, img_num, rotate=False)
            total = np.zeros(img_num, np.float32)
            for f in range(ms.shape[0]):
                total += ms[f]
            score[s], video[s] = (a[0] for a in cvt_amd.topk_select(total[None, :], k))
        return score, video

    for k in KS:
        print("# %d,%d,%d: index built, k = %d" % (img_num, frames, videos, k), file=sys.stderr, flush=True)
        h = ix.rank_videos(qh, seg, NPROBE, img_num, k, rotate=False)
        last = ix.last_rank()
        d = tuple(o.cpu().numpy() for o in ix.rank_videos(qd, seg, NPROBE, img_num, k, rotate=False))
        th = timed(lambda: ix.rank_videos(qh, seg, NPROBE, img_num, k, rotate=False), sync)
        td = timed(lambda: ix.rank_videos(qd, seg, NPROBE, img_num, k, rotate=False), sync)
        if args.device_only:
            tp, equal = (float("nan"), float("nan")), "-"
        else:
            p = parent(k)
            print("# %d,%d,%d: the parent's way ran once" % (img_num, frames, videos), file=sys.stderr, flush=True)
            equal = "yes" if all(np.array_equal(p[0].view(np.uint32), o[0].view(np.uint32)) and np.array_equal(p[1], o[1]) for o in (h, d)) else "NO"
            tp = timed(lambda: parent(k), sync)
        saved = nq * img_num * 4 + videos * img_num * 4 - videos * k * 12
        # the kernel reads every score cell once and writes a segment's totals once per chunk it has frames in (and reads them back
        # in every chunk but its first)
        rows = 0
        for c0 in range(0, nq, int(last["frames_per_chunk"])):
            c1 = min(nq, c0 + int(last["frames_per_chunk"]))
            for s in range(c0 // frames, (c1 - 1) // frames + 1):
                rows += 1 + (1 if seg[s] < c0 else 0)
        fold = (nq + rows) * img_num * 4
        print("%9d %6d %6d %4d | %10.3f %10.3f | %10.3f %10.3f | %10.3f %10.3f | %7.2f %7.2f | %5s | %8.1fMB %8.3f %6d" % (
            img_num, frames, videos, k, tp[0], tp[1], th[0], th[1], td[0], td[1], tp[0] / th[0], tp[0] / td[0], equal, saved / 1e6, fold / 1e9,
            last["chunks"]), flush=True)
        if equal == "NO":
            sys.exit(3)
    ix.close()


if args.point:
    point(*(int(v) for v in args.point.split(",")))
    sys.exit(0)

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


say("# rank_videos_sweep: %d coarse lists, M = %d, K = %d, %d entries per video, %d lists probed; times in ms of whole calls from the host" % (
    LISTS, M, K, PER_VIDEO, NPROBE))
say(HEADER)
failed = 0
for img_num in IMG_NUMS:
    for frames in FRAMES:
        for videos in VIDEOS:
            limit = 150 + (400 if img_num * frames * videos >= 5 * 10 ** 8 else 0)
            try:
                # (the point's notes on stderr pass through as they come: a long point is not silent)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--point", "%d,%d,%d" % (img_num, frames, videos)], stdout=subprocess.PIPE,
                                   text=True, timeout=limit)
                rc, out, err = r.returncode, r.stdout, "see its notes on stderr"
            except subprocess.TimeoutExpired as e:
                rc, out, err = 124, (e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or ""), "time limit of %d s" % limit
            for l in out.splitlines():
                say(l)
            if rc != 0:
                say("# point %d,%d,%d failed with status %d: %s" % (img_num, frames, videos, rc, err.strip()[-600:]))
                failed = rc
                break
        if failed:
            break
    if failed:
        break
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(1 if failed else 0)
