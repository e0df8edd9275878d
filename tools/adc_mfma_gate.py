#!/usr/bin/env python3
"""The measurement behind profiles/adc_mfma_gate.txt: the uint8 flat engine (cvtmi_flat_search_dev, L2, path 4) at the headline's shape --
1 M x 128-d rows, 1024 and 10 000 queries, top-100 -- timed with events, ten repetitions.  Compare with a plain bench.py run on the same box."""
import os, sys, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import cvt_amd

torch.cuda.set_device(0)
g = torch.Generator(device="cuda"); g.manual_seed(1)
n, D, nq, k = 1_000_000, 128, 10_000, 100
# SIFT-like bytes: clipped gaussian around 40
x = (torch.randn((n, D), generator=g, device="cuda") * 30 + 40).clamp_(0, 255).to(torch.uint8)
q = (torch.randn((nq, D), generator=g, device="cuda") * 30 + 40).clamp_(0, 255).to(torch.uint8)
ix = cvt_amd.FlatIndex(2, D)
ix.add(x)
out = {}
for nqs in (1024, 10_000):
    qq = q[:nqs].contiguous()
    for _ in range(3):
        ix.search(qq, k)
    torch.cuda.synchronize()
    path = ix.last_search()
    ts = []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); ix.search(qq, k); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    out["nq=%d" % nqs] = {"path": path[0], "ms_min": round(ts[0], 4), "ms_median": round(ts[5], 4), "ms_max": round(ts[-1], 4)}
    print("flat u8 L2 1M x 128, nq=%d k=%d: path %d, ms min/med/max %.4f %.4f %.4f" % (nqs, k, path[0], ts[0], ts[5], ts[-1]), flush=True)
print(json.dumps(out))
