#!/usr/bin/env python3
"""PCA training (cvtmi_pca_covariance / cvtmi_pca_train) at the reference's model shapes, with a numpy float64 CPU baseline.

Device events around the _dev entries, after warm-up calls:
  covariance  cvtmi_pca_covariance_dev: the mean pass, the centred covariance and its reduction (scratch allocation included)
  whole       cvtmi_pca_train_dev: the above, rocsolver_dsyevd and the finish kernel
  eig         whole - covariance
The mean pass alone and the covariance kernel alone come from a `rocprofv3 --kernel-trace --stats` run of this script
(pca_colsum_kernel + pca_mean_kernel; pca_cov_kernel).  fp64 flop of the covariance: n * din * (din + 1) (the tiles on
and below the diagonal, counted as if only the lower triangle were computed).
CPU baseline: numpy float64 d^T d and numpy.linalg.eigh on a row subset of the same rows (--cpu-rows); OpenCV, which the
reference trains with, is not installed, so it is not measured.

  python tools/bench_pca_train.py [--reps R] [--cpu-rows N] [--shapes all|small]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cvt_amd  # noqa: E402

SHAPES = [(1 << 20, 1024, 128), (5_000_000, 2048, 256), (1 << 20, 128, 64)]


def ev_time(f, reps):
    f()  # warm-up (first launches, solver handle, library load)
    f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-rows", type=int, default=1 << 18)
    ap.add_argument("--shapes", default="all")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev); g.manual_seed(11)
    print("device %s, %d CUs; host %d cores (os.cpu_count), numpy %s" % (
        torch.cuda.get_device_name(dev), torch.cuda.get_device_properties(dev).multi_processor_count, os.cpu_count(), np.__version__))
    shapes = SHAPES if a.shapes == "all" else [s for s in SHAPES if s[0] * s[1] <= (1 << 30)]
    for n, din, dout in shapes:
        x = torch.randn((n, din), generator=g, device=dev).relu_()
        x.mul_(torch.rand((1, din), generator=g, device=dev) + 0.5)
        cov_ms = ev_time(lambda: cvt_amd.pca_covariance(x), a.reps)
        whole_ms = ev_time(lambda: cvt_amd.pca_train(x, dout), a.reps)
        flop = float(n) * din * (din + 1)
        print("pca_train %8d x %4d -> %3d: covariance call %.3f ms (%.1f TFLOP/s fp64 on n*din*(din+1) flop, %.2f TB/s of rows read twice), "
              "eig+finish %.3f ms, whole call %.3f ms" % (n, din, dout, cov_ms, flop / cov_ms / 1e9, 2.0 * n * din * 4 / cov_ms / 1e9,
                                                          whole_ms - cov_ms, whole_ms))
        if a.cpu_rows > 0:
            m = min(n, a.cpu_rows)
            xs = x[:m].cpu().numpy()
            t0 = time.perf_counter()
            mu = xs.astype(np.float64).mean(axis=0)
            d = (xs - mu.astype(np.float32)).astype(np.float64)
            c = d.T @ d / m
            t1 = time.perf_counter()
            np.linalg.eigh(c)
            t2 = time.perf_counter()
            print("  cpu numpy float64, %d of the rows, %d cores: mean + d^T d %.1f ms, eigh %.1f ms" % (m, os.cpu_count(), (t1 - t0) * 1e3,
                                                                                                       (t2 - t1) * 1e3))
            del xs, d, c
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
