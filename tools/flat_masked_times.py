#!/usr/bin/env python3
"""cvtmi_flat_search_masked_dev against cvtmi_flat_search_dev under "flat_variant" 1 (the exact kernels the masked search is made of),
on the same handle, alternating in one process.

  k = 10; 1 M x 128-d fp32 L2 and 10 M x 512-byte uint8 L2; 1 / 16 / 1000 queries;
  masks: all ones, random 1 %, random 0.1 %, all zero (nothing to score: the floor of the compaction and the launches);
  the sparse masks once more with "masked_parts" forced to 1, 8 and 64: is the default plan, made for a mask that allows every row,
  wrong for them?
Timing: device events around CALLS calls on one stream (CALLS sized so that a window takes about WINDOW seconds, at least 3), after a
warm-up of every configuration; the configurations take turns REPS times; median, min and max per call.  MEASURED: the times.
MODELLED: the bytes -- the mask words + 4 bytes per allowed row written and read as the list + the allowed rows (fp32 rows live in 64-row
blocks: an allowed row whose block neighbours are not allowed still costs whole 128-byte lines, which the model does not count) -- once
per query group, and hence the bytes per second printed beside the dense case.

  ROWS_F32 / ROWS_U8 / NQS / K / REPS / WINDOW in the environment change the shapes."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import cvt_amd

dev = torch.device("cuda", 0)
REPS = int(os.environ.get("REPS", 5))
WINDOW = float(os.environ.get("WINDOW", 0.25))
K = int(os.environ.get("K", 10))
NQS = [int(v) for v in os.environ.get("NQS", "1,16,1000").split(",")]
SHAPES = [("fp32 L2", 1, int(os.environ.get("ROWS_F32", 1_000_000)), 128), ("uint8 L2", 2, int(os.environ.get("ROWS_U8", 10_000_000)), 512)]


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def words_of(allowed):
    """bool [n] on the device -> int64 words, bit r & 63 of word r >> 6 = row r"""
    pad = (-allowed.shape[0]) % 64
    bits = torch.nn.functional.pad(allowed.to(torch.int64), (0, pad)).reshape(-1, 64)
    return (bits << torch.arange(64, device=allowed.device, dtype=torch.int64)).sum(dim=1).contiguous()


def main():
    assert torch.cuda.is_available(), "needs the GPU: there is no fallback"
    cvt_amd.set_tuning("flat_variant", 1)
    g = torch.Generator(device=dev)
    g.manual_seed(13)
    for name, metric, n, D in SHAPES:
        if n <= 0:
            continue
        rb = D if metric == 2 else 4 * D
        if metric == 2:
            x = torch.randint(0, 256, (n, D), generator=g, device=dev, dtype=torch.uint8)
        else:
            x = torch.randn((n, D), generator=g, device=dev)
        ix = cvt_amd.FlatIndex(metric, D)
        ix.add(x)
        del x
        torch.cuda.empty_cache()
        masks = {}
        for label, share in (("all ones", 1.0), ("1 %", 0.01), ("0.1 %", 0.001), ("all zero", 0.0)):
            allowed = torch.rand(n, generator=g, device=dev) < share
            masks[label] = (words_of(allowed), int(allowed.sum()))
        print("%s  %d x %d  (%.2f GB of rows), k = %d" % (name, n, D, n * rb / 1e9, K), flush=True)
        for nq in NQS:
            q = torch.randint(0, 256, (nq, D), generator=g, device=dev, dtype=torch.uint8) if metric == 2 else torch.randn((nq, D), generator=g, device=dev)
            configs = [("cvtmi_flat_search (flat_variant 1)", 0, None, lambda: ix.search(q, K))]
            for label, (w, cnt) in masks.items():
                configs.append(("masked, %s" % label, 0, cnt, lambda w=w: ix.search_masked(q, K, w)))
            for label in ("1 %", "0.1 %"):
                for parts in (1, 8, 64):
                    w, cnt = masks[label]
                    configs.append(("masked, %s, masked_parts %d" % (label, parts), parts, cnt, lambda w=w: ix.search_masked(q, K, w)))
            calls, series, plans = [], [[] for _ in configs], []
            for _, parts, _, fn in configs:            # warm-up of every configuration, and the size of its window
                ix.set_param("masked_parts", parts)
                timed(fn, 2)
                calls.append(max(3, min(2000, int(WINDOW * 1e3 / max(timed(fn, 3), 1e-3)))))
                plans.append(ix.last_masked())
            route = ix.last_search()[0]                # (of the plain search: the masked ones do not touch it)
            for _ in range(REPS):                      # the configurations take turns
                for c, (_, parts, _, fn) in enumerate(configs):
                    ix.set_param("masked_parts", parts)
                    series[c].append(timed(fn, calls[c]))
            ix.set_param("masked_parts", 0)
            print("  nq = %d" % nq)
            groups = (nq + 3) // 4 if nq >= 4 else nq
            for c, (label, _, cnt, _) in enumerate(configs):
                ts = series[c]
                med = statistics.median(ts)
                line = "    %-40s median %9.4f ms  (min %9.4f, max %9.4f, %d x %d calls)" % (label, med, min(ts), max(ts), len(ts), calls[c])
                if cnt is None:
                    model = groups * n * rb
                    line += "   route %d; modelled %.2f GB, %.2f TB/s" % (route, model / 1e9, model / 1e12 / (med / 1e3))
                else:
                    model = (n + 63) // 64 * 8 + 4 * cnt + groups * cnt * (rb + 4)
                    line += "   qt %d, %d parts; %d rows allowed; modelled %.3f GB, %.2f TB/s" % (plans[c][0], plans[c][1], cnt, model / 1e9, model / 1e12 / (med / 1e3))
                print(line, flush=True)
        ix.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
