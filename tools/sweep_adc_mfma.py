#!/usr/bin/env python3
"""Where does the int8 matrix-core bound filter ("scan_mfma", cvt_amd/csrc/adc_mfma.hip) pass the ADC scan?  Batch size x index size, the
bench's data (SIFT-like rows, dense rotation, codebooks trained on a 100 K-row sample), top-100: milliseconds per search of the route and
of the scan on the same handle, and how many queries of the batch the route handed to the exact scan.  The defaults of
"scan_mfma_min_nq" / "scan_mfma_min_rows" come from this table (profiles/adc_mfma_sweep.txt).

    python tools/sweep_adc_mfma.py [--rows 262144,1000000,4000000] [--nq 256,512,1024,2048,4096,10000] [--k 100] [--sample 2]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, M, K = 128, 16, 256


def timed(torch, fn, reps):
    fn(); fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="262144,1000000,4000000")
    ap.add_argument("--nq", default="256,512,1024,2048,4096,10000")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--sample", default="2")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import cvt_amd
    from cvt_amd import synth
    torch.cuda.set_device(0)
    R = synth.random_rotation(D, seed=7)
    zero = np.zeros((1, D), np.float32)
    tmp = cvt_amd.OpqIndex(zero, np.zeros((M, K, D // M), np.float32), R=R)
    books = synth.train_books(tmp.rotate(synth.sift_like(100_000, D, seed=0xC0FFEE, device="cuda")), M, K, iters=4).astype(np.float32)
    tmp.close()
    nqs = [int(v) for v in args.nq.split(",")]
    q_all = synth.sift_like(max(nqs), D, seed=0xBEEF, device="cuda")
    print("rows nq k sample route_ms scan_ms scan/route flagged")
    for rows in (int(v) for v in args.rows.split(",")):
        ix = cvt_amd.OpqIndex(zero, books, R=R)
        for a in range(0, rows, synth.CHUNK * 4):
            b = min(rows, a + synth.CHUNK * 4)
            _, codes = ix.rotate_encode(synth.sift_like(b - a, D, seed=0xC0FFEE, row_begin=a, device="cuda"))
            ix.add_codes(codes)
        ix.set_param("scan_mfma_min_nq", 1); ix.set_param("scan_mfma_min_rows", 1); ix.set_param("profile", 1)
        for nq in nqs:
            q = q_all[:nq].contiguous()
            ix.set_param("scan_mfma", 0)
            scan_ms = timed(torch, lambda: ix.search(q, args.k), args.reps)
            ref = ix.search(q, args.k)
            ix.set_param("scan_mfma", 1)
            for sample in (int(v) for v in args.sample.split(",")):
                ix.set_param("scan_mfma_sample", sample)
                route_ms = timed(torch, lambda: ix.search(q, args.k), args.reps)
                got = ix.search(q, args.k)
                stat = ix.last_mfma()
                same = torch.equal(got[1], ref[1]) and torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32))
                print("%d %d %d %d %.4f %.4f %.3f %d%s" % (rows, nq, args.k, sample, route_ms, scan_ms, scan_ms / route_ms, stat[1],
                                                         "" if same and stat[0] == nq else "  MISMATCH or route not taken %r" % (stat,)), flush=True)
        ix.close()


if __name__ == "__main__":
    main()
