#!/usr/bin/env python3
"""CPU model of the int8 bound filter of the ADC search (cvt_amd/csrc/adc_mfma.hip), no GPU part: SIFT-like rows and 64 queries, the bench's
rotation, a 4-iteration numpy Lloyd codebook on a 100 K-row sample (NOT the library's k-means: the figures are indicative).  Prints, for the
per-row-norm and the codebook-maxima form of the Cauchy-Schwarz bound E: E / tau, the true error of the int8 score, the rows per query that
survive the FINAL threshold (the k-th smallest upper bound over all rows) and a SAMPLED one (the k-th smallest of the minima of the upper
bound over 4096 disjoint row sets, over all rows and over every 8th row).  The route's own sample (every second tile group, 1024 to 4096
sets) is not modelled here; what it passes is measured on the device (profiles/adc_mfma_sweep.txt).

    python tools/model_adc_i8.py [rows]"""
import sys, time, numpy as np, torch
import os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvt_amd import synth
torch.manual_seed(0)
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
NQ, K, M, D, TOPK = 64, 256, 16, 128, 100
t0 = time.time()
R = torch.from_numpy(synth.random_rotation(D, seed=7))
x = synth.sift_like(N, D, seed=0xC0FFEE, device='cpu')
q = synth.sift_like(NQ, D, seed=0xBEEF, device='cpu')
xr = x @ R.T; qr = q @ R.T
print('data', time.time() - t0, flush=True)
# books: Lloyd on a 100k sample, 4 iterations
samp = synth.sift_like(100_000, D, seed=0xC0FFEE, device='cpu') @ R.T
st = D // M
books = torch.empty(M, K, st)
for m in range(M):
    s = samp[:, m*st:(m+1)*st]
    c = s[torch.randperm(s.shape[0])[:K]].clone()
    for it in range(4):
        a = torch.cdist(s, c).argmin(1)
        for j in range(K):
            sel = s[a == j]
            if sel.shape[0]: c[j] = sel.mean(0)
    books[m] = c
print('books', time.time() - t0, flush=True)
codes = torch.empty(N, M, dtype=torch.int64)
for m in range(M):
    for a in range(0, N, 200_000):
        codes[a:a+200_000, m] = torch.cdist(xr[a:a+200_000, m*st:(m+1)*st], books[m]).argmin(1)
xh = torch.cat([books[m][codes[:, m]] for m in range(M)], 1).double()   # decoded rows
print('encode', time.time() - t0, flush=True)
qd = qr.double()
adc = (qd*qd).sum(1)[:, None] + (xh*xh).sum(1)[None] - 2*qd @ xh.T      # [NQ][N]
tau = adc.kthvalue(TOPK, dim=1).values
print('adc kth: mean %.4f  1st %.4f  median-of-all %.4f' % (tau.mean(), adc.min(1).values.mean(), adc.median(1).values.mean()))
for mul in (1.02, 1.05, 1.1, 1.2):
    print(' rows within %.2f x tau: %.1f per query' % (mul, (adc <= tau[:, None]*mul).sum(1).double().mean()))
# int8 operands
bk = books.double()
lo = torch.cat([bk[m].min(0).values for m in range(M)]); hi = torch.cat([bk[m].max(0).values for m in range(M)])
def run(name, s, c, per_query_t, qclip=None):
    Xf = (xh - c) / s
    X = Xf.round().clamp(-127, 127); eps = Xf - X
    w = qd * s
    if per_query_t: t = w.abs().max(1).values[:, None] / 127.0
    else: t = torch.full((NQ, 1), float(qclip) / 127.0, dtype=torch.float64)
    Wf = w / t; W = Wf.round().clamp(-127, 127); dl = Wf - W
    score = t * (W @ X.T) + (qd @ c)[:, None]
    n = (xh*xh).sum(1)
    Xn = X.norm(dim=1); en = eps.norm(dim=1)
    qq = (qd*qd).sum(1)[:, None]
    mid = qq + n[None] - 2*score
    true_err = (adc - mid).abs()
    for kind in ('per-row norms', 'global maxima'):
        if kind == 'per-row norms': E = 2*(t*dl.norm(dim=1)[:, None]*Xn[None] + w.norm(dim=1)[:, None]*en[None])
        else: E = 2*(t*dl.norm(dim=1)[:, None]*Xn.max() + w.norm(dim=1)[:, None]*en.max()).expand(NQ, N)
        assert bool((true_err <= E + 1e-9).all())
        LB = mid - E; UB = mid + E
        final = (LB <= tau[:, None]).sum(1).double()
        # sampled threshold: 4096 disjoint row sets (strided), min UB of each, the k-th smallest
        ns = 4096; L = N // ns * ns
        for frac, lab in ((1, 'all rows'), (8, 'every 8th row')):
            sub = UB[:, :L:frac]; Ls = sub.shape[1] // ns * ns
            mins = sub[:, :Ls].reshape(NQ, Ls // ns, ns).min(1).values
            ts = mins.kthvalue(TOPK, dim=1).values
            surv = (LB <= ts[:, None]).sum(1).double()
            print('%-34s %-14s E/tau %.3f true|err|/tau mean %.4f max %.4f | survivors final-thr mean %.0f max %.0f | sampled(%s) mean %.0f max %.0f'
                  % (name, kind, (E.mean(1)/tau).mean(), (true_err.mean(1)/tau).mean(), (true_err.max(1).values/tau).mean(), final.mean(), final.max(), lab, surv.mean(), surv.max()), flush=True)
s_dim = ((hi - lo) / 254).clamp_min(1e-12); c_dim = (hi + lo) / 2
run('per-dim scale, per-query t', s_dim, c_dim, True)
wmax = (qd * s_dim).abs().max()
run('per-dim scale, one t (batch max)', s_dim, c_dim, False, wmax)
s_g = torch.full((D,), float(((hi - lo).max()) / 254), dtype=torch.float64)
run('one scale, per-query t', s_g, c_dim, True)
print('done', time.time() - t0)
