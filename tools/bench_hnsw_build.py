#!/usr/bin/env python3
"""HNSW construction on the GPU (cvtmi_hnsw_build, batch-synchronous) against the host build (hnsw_build CLI, addPoints on
THREADS host threads) of the same rows, and the recall of both graphs.  Cases: the config-5 graph (1 M x 128-d clustered,
normalised, M = 16, ef_construction = 40, IP), a 200 K L2 graph of the same generator, and a schedule sweep on the 200 K rows.
Writes profiles/hnsw_build.txt (OUT=... to change).  GPU times are warmed and device-synchronised; the phase split comes from
set_tuning("hnsw_build_phases", 1) in a separate run."""
import os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import cvt_amd

THREADS = int(os.environ.get("THREADS", 16))
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "hnsw_build.txt"))
N1 = int(os.environ.get("ROWS", 1_000_000))
SWEEP = os.environ.get("SWEEP", "1") != "0"
lines = []


def log(s):
    print(s, flush=True)
    lines.append(s)


def rows(n, D=128, nq=1000):
    rng = np.random.default_rng(5)   # the config-5 generator (bench.py)
    cen = rng.normal(size=(1000, D)).astype(np.float32)
    x = cen[rng.integers(0, 1000, n)] + 0.6 * rng.normal(size=(n, D)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = x[rng.integers(0, n, nq)] + 0.15 * rng.normal(size=(nq, D)).astype(np.float32)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(x, np.float32), q


def truth(x, q, metric):
    xd, qd = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
    if metric == 0:
        return torch.topk(qd @ xd.T, 10, dim=1).indices.cpu().numpy()
    return torch.topk(-torch.cdist(qd, xd), 10, dim=1).indices.cpu().numpy()


def recall(idx, q, t, ef):
    _, lab = idx.search(q, 10, ef)
    r1 = float((lab[:, 0] == t[:, 0]).mean())
    r10 = float(np.mean([len(set(lab[i]) & set(t[i])) / 10.0 for i in range(len(q))]))
    return r1, r10


def gpu_build(xd, metric, M, efc, max_batch=0):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx = cvt_amd.hnsw_build(xd, metric, M, efc, max_batch=max_batch)
    torch.cuda.synchronize()
    return idx, time.perf_counter() - t0


def host_build(x, metric, M, efc, tmp):
    rf = os.path.join(tmp, "rows.bin"); x.tofile(rf)
    out = os.path.join(tmp, "host.hnsw")
    t0 = time.perf_counter()
    subprocess.run([os.path.join(ROOT, "cvt_amd", "bin", "hnsw_build"), rf, str(x.shape[1]), str(M), str(efc), out,
                    "l2" if metric == 1 else "ip", "-", str(THREADS)], check=True, capture_output=True)
    t = time.perf_counter() - t0
    return cvt_amd.HnswIndex(open(out, "rb").read(), metric, x.shape[1]), t


def case(name, x, q, metric, M, efc, tmp):
    D = x.shape[1]
    xd = torch.from_numpy(x).cuda()
    t = truth(x, q, metric)
    gpu_build(xd[:20000].contiguous(), metric, M, efc)   # warm-up: module load, first allocations
    g, tg = gpu_build(xd, metric, M, efc)
    cvt_amd.set_tuning("hnsw_build_phases", 1)
    g2, tg2 = gpu_build(xd, metric, M, efc)
    ph = cvt_amd.hnsw_build_phases()
    cvt_amd.set_tuning("hnsw_build_phases", 0)
    same = g.save() == g2.save()
    del g2
    h, th = host_build(x, metric, M, efc, tmp)
    log("%s: %d x %d-d, %s, M=%d efc=%d" % (name, x.shape[0], D, "IP" if metric == 0 else "L2", M, efc))
    log("  GPU build (default schedule) %.2f s   host build (%d threads) %.2f s   speed-up %.1fx   repeat build identical: %s" % (
        tg, THREADS, th, th / tg, same))
    log("  GPU phases (timed run, %.2f s): traversal %.0f ms, selection %.0f ms, back links %.0f ms, %d batches, host %.0f ms, "
        "no per-batch host sync" % (tg2, ph[0], ph[1], ph[2], ph[3], ph[4]))
    for ef in (64, 1000):
        rg, rh = recall(g, q, t, ef), recall(h, q, t, ef)
        log("  ef=%4d  recall@1 / @10: GPU graph %.4f / %.4f   host graph %.4f / %.4f" % (ef, rg[0], rg[1], rh[0], rh[1]))
    return g, h


def main():
    with tempfile.TemporaryDirectory() as tmp:
        log("# tools/bench_hnsw_build.py -- cvtmi_hnsw_build vs the hnsw_build CLI on %d host threads, same box" % THREADS)
        x, q = rows(N1)
        case("config-5 graph", x, q, 0, 16, 40, tmp)
        del x
        x2, q2 = rows(200_000)
        case("200K L2", x2, q2, 1, 16, 40, tmp)
        if SWEEP:
            log("schedule sweep, 200K x 128-d IP, M=16 efc=40 (batch <= inserted / frac, <= cap):")
            t = truth(x2, q2, 0)
            xd = torch.from_numpy(x2).cuda()
            for frac, cap in ((8, 8192), (16, 8192), (32, 8192), (64, 8192), (32, 2048), (32, 32768)):
                cvt_amd.set_tuning("hnsw_build_frac", frac)
                cvt_amd.set_tuning("hnsw_build_cap", cap)
                g, tg = gpu_build(xd, 0, 16, 40)
                r = recall(g, q2, t, 64)
                log("  frac 1/%-3d cap %5d: %.3f s  recall@1 %.4f  recall@10 %.4f (ef=64)" % (frac, cap, tg, r[0], r[1]))
            cvt_amd.set_tuning("hnsw_build_frac", 32)
            cvt_amd.set_tuning("hnsw_build_cap", 8192)
            h, th = host_build(x2, 0, 16, 40, tmp)
            r = recall(h, q2, t, 64)
            log("  host build (%d threads): %.3f s  recall@1 %.4f  recall@10 %.4f (ef=64)" % (THREADS, th, r[0], r[1]))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
