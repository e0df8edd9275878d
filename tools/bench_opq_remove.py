"""Removal from a large OPQ index (cvtmi_opq_remove_videos) against the only route there was before it:
get_entries -> host filter -> reset -> add_codes.

    python tools/bench_opq_remove.py [--n 100000000] [--per-video 100] [--out profiles/opq_remove.txt]

10^8 entries of M = 16 code bytes in coarseK = 8192 lists, 10^6 videos of 100 entries.  Timed: a call that drops nothing (mark +
scan alone), a random 10 % of the videos, a single video at the end / in the middle / at the start of the index (rows before the
first dropped entry are not moved), the rebuild of the derived copies by the first search afterwards (the price every append
pays too), and the round trip through the host over the same set.  Device events around the call and the host clock; the
algorithmic bytes of the call (4 n for the mark; (M + 8) n read and (M + 8) kept written for the move) as a fraction of 8 TB/s."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, M, K, L = 128, 16, 256, 8192
PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--per-video", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=0, help='"remove_chunk" (0 = the default)')
    ap.add_argument("--no-round-trip", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import cvt_amd
    n, per = a.n, a.per_video
    nvid = (n + per - 1) // per
    rng = np.random.default_rng(1)
    coarse = (rng.normal(size=(L, D)) * 0.1).astype(np.float32)
    books = (rng.normal(size=(M, K, D // M)) * 0.03).astype(np.float32)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def build():
        idx = cvt_amd.OpqIndex(coarse, books)
        if a.chunk:
            idx.set_param("remove_chunk", a.chunk)
        idx.reserve(n)
        g = torch.Generator(device="cuda")
        g.manual_seed(2)
        piece = 10_000_000
        for lo in range(0, n, piece):
            m = min(piece, n - lo)
            codes = torch.randint(0, 256, (m, M), dtype=torch.uint8, device="cuda", generator=g)
            lists = torch.randint(0, L, (m,), dtype=torch.int32, device="cuda", generator=g)
            vids = (torch.arange(lo, lo + m, device="cuda") // per).to(torch.int32)
            idx.add_codes(codes, lists, vids)
        torch.cuda.synchronize()
        return idx

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return r, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    def report(tag, n0, removed, dev_ms, host_ms, moved=True):
        kept = n0 - removed
        b = 4 * n0 + ((M + 8) * (n0 + kept) if moved else 0)
        say("%-34s n %11d  dropped %9d  device %9.3f ms  host %9.3f ms  %6.2f ms per million entries  %7.3f GB algorithmic = %5.1f %% of 8 TB/s"
            % (tag, n0, removed, dev_ms, host_ms, dev_ms / (n0 / 1e6), b / 1e9, 100.0 * b / (dev_ms * 1e-3) / PEAK))

    q = torch.from_numpy((rng.normal(size=(8, D)) * 0.1).astype(np.float32)).cuda()

    def rebuild_cost(idx):
        _, first, _ = timed(lambda: idx.search_ivf(q, 8, 10))
        _, second, _ = timed(lambda: idx.search_ivf(q, 8, 10))
        say("%-34s first search_ivf %9.3f ms, second %9.3f ms: rebuild of the list-ordered copy %9.3f ms" % ("", first, second, first - second))

    say("# cvtmi_opq_remove_videos: n = %d, M = %d, coarseK = %d, %d videos of %d entries, remove_chunk %s" % (n, M, L, nvid, per, a.chunk or "default"))
    idx = build()
    idx.search_ivf(q, 8, 10)                                                        # the derived copies exist, as in service
    absent = torch.tensor([nvid + 5], dtype=torch.int32, device="cuda")
    timed(lambda: idx.remove_videos(absent))                                        # (first call: allocates the scratch)
    r, dms, hms = timed(lambda: idx.remove_videos(absent))
    report("nothing dropped (mark + scan)", n, r, dms, hms, moved=False)
    gone = torch.randperm(nvid, device="cuda")[:nvid // 10].to(torch.int32)
    r, dms, hms = timed(lambda: idx.remove_videos(gone, renumber=True))
    report("random 10 % of the videos", n, r, dms, hms)
    rebuild_cost(idx)
    idx.close()
    del idx
    idx = build()
    idx.search_ivf(q, 8, 10)
    timed(lambda: idx.remove_videos(absent))
    for tag, v in (("one video, the last", nvid - 1), ("one video, the middle", nvid // 2), ("one video, the first", 0)):
        n0 = idx.ntotal
        r, dms, hms = timed(lambda: idx.remove_videos(torch.tensor([v], dtype=torch.int32, device="cuda")))
        report(tag, n0, r, dms, hms)
    rebuild_cost(idx)
    if not a.no_round_trip:
        gone_h = gone.cpu().numpy()
        n0 = idx.ntotal
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        off, vid, codes = idx.get_entries()
        t1 = time.perf_counter()
        keep = ~np.isin(vid, gone_h)
        lists = np.repeat(np.arange(L, dtype=np.int32), np.diff(off))
        codes, lists, vid = codes[keep], lists[keep], vid[keep]
        t2 = time.perf_counter()
        idx.reset()
        idx.add_codes(codes, lists, vid)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        say("%-34s n %11d  dropped %9d  get_entries %9.1f ms + host filter %9.1f ms + reset / add_codes %9.1f ms = %9.1f ms  (insertion order lost)"
            % ("round trip through the host", n0, n0 - idx.ntotal, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3))
    idx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
