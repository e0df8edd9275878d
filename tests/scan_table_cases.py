"""Inputs at the edges of the ADC scans' 15-bit lower-bound tables, shared by test_scan_table_regimes.py (which pins
each case to the regime its name claims, on the CPU) and test_gpu_opq_scan_tables.py (which runs the kernels on them).

Every fast scan quantises each query's fp32 distance tables with the query's own scale / bias / slack (adc_scan16.h
scan16_query_params / scan16_quantise, called by scan16q_build_tables and adc_scan_h.hip scan16h_prep_kernel).  `classify` derives the
same quantities from the oracle's tables, one fp32 operation at a time, so the predicates are conditions on the INPUTS:
nothing of the library is loaded here.

A case is (books, queries, codes), built from seeds.  "xS" multiplies books AND queries by np.float32(S): the table
entries scale with S * S.  Every single-regime case has NQ = 9 queries (one full query group and a ragged one), all of
them in the regime; `mixed` puts nine different regimes side by side over plain books."""
import contextlib
import math
import os
import re

import numpy as np

SEED = 8
NQ = 9
ROWS = 6000 + 7            # past the 2048-row seed region, no multiple of 64
ROWS_BIG = 65536 + 71      # the small-batch path and the k > 128 filter scan start at 65 536 rows
MAXSUM = 32766             # adc_scan16.h SQ_MAXSUM
FLT_MIN = np.float32(1.17549435e-38)   # smallest normal fp32

SCALED = {"x1e-16": 1e-16, "x1e-17": 1e-17, "x1e-18": 1e-18, "x1e-20": 1e-20, "x1e-22": 1e-22, "x1e-23": 1e-23,
          "x5e18": 5e18, "x1e19": 1e19, "x1.5e19": 1.5e19, "x2.5e19": 2.5e19}
CASES = ["constant", "one_live"] + list(SCALED) + ["shift3000", "shift1e4", "dominant"]
ONE_LIVE_M = 5             # the sub-quantiser that keeps its codewords in `one_live`
MIXED_CODEWORD = 7         # mixed[1] sits on this codeword of every sub-quantiser
# the three cases repeated at other sub-vector lengths (the table kernels have a step == 8 path and a generic one)
STEP_CASES = ["x1e-18", "x1e19", "shift1e4"]
STEP_DIMS = [64, 256]      # M = 16: step 4 and step 16


def synth_model(rng, D, M, K, n_train=4000, scale=1.0):
    """codebooks drawn from normal training rows, as the scan tests of test_gpu_opq.py draw them"""
    x = (rng.normal(size=(n_train, D)) * scale).astype(np.float32)
    step = D // M
    books = np.stack([x[rng.integers(0, n_train, K), m * step:(m + 1) * step] for m in range(M)]).astype(np.float32)
    return np.ascontiguousarray(books)


def _base(D, M, K, rows, seed):
    rng = np.random.default_rng(seed)
    books = synth_model(rng, D, M, K, scale=0.1)
    q = (rng.normal(size=(NQ, D)) * 0.1).astype(np.float32)
    codes = rng.integers(0, K, size=(rows, M), dtype=np.uint8)   # (drawn last: every row count has the same books and queries)
    return books, q, codes


def _tables(books, q):
    """fp32 tables [M][K] of one query, the reference's arithmetic (sum over the sub-vector ascending of fl(fl(q - c)^2)): what
    orc.lut returns for a zero centroid; here so that the offset search below needs no oracle"""
    M, K, step = books.shape
    acc = np.zeros((M, K), np.float32)
    with np.errstate(all="ignore"):
        for kk in range(step):
            t = (q.reshape(M, step)[:, kk][:, None] - books[:, :, kk]).astype(np.float32)
            acc = (acc + (t * t).astype(np.float32)).astype(np.float32)
    return acc


def classify(lut):
    """The quantities the three table builders derive from one query's fp32 tables lut[M][K]; fp32 where they use fp32."""
    lut = np.ascontiguousarray(lut, dtype=np.float32)
    M = lut.shape[0]
    finite = np.isfinite(lut)
    f32 = np.float32
    with np.errstate(all="ignore"):
        mn = np.zeros(M, np.float32); mx = np.zeros(M, np.float32)
        for m in range(M):
            if finite[m].any():
                mn[m] = lut[m][finite[m]].min(); mx[m] = lut[m][finite[m]].max()
        rng_ = f32(0.0)
        bias = 0.0
        for m in range(M):
            rng_ = f32(rng_ + f32(mx[m] - mn[m]))
            bias += float(mn[m])
        pre = f32(f32(rng_ / f32(MAXSUM)) * f32(1.001)) if rng_ > 0 else f32(1.0)
        scale = pre if pre > f32(1e-37) else f32(1e-37)
        inv = f32(f32(1.0) / scale)
        sl = 34.0 + math.ceil(4e-6 * (32767.0 + bias * float(inv)))
        # the 15-bit entries: max(0, floor((v - mn) * inv) - 1), non-finite -> 0
        f = ((lut - mn[:, None]).astype(np.float32) * inv).astype(np.float32)
        qv = np.where(finite, np.clip(np.floor(np.where(finite, f, 0)).astype(np.int64) - 1, 0, MAXSUM), 0)
    return dict(mn=mn, mx=mx, range=rng_, bias=bias, pre_clamp=pre, scale=scale, inv=inv, sl=sl,
                nonfinite=bool((~finite).any()), lazy=bool(not (~finite).any() and sl < 1024.0 and bias >= 0.0),
                qv=qv, max_int_sum=int(qv.max(axis=1).sum()))


def _shift_for_window(books, q, lo, hi, start):
    """`books + offset` with the slack of every query inside [lo, hi): the slack grows linearly with the offset (bias ~ offset^2,
    range ~ offset), so a few proportional steps from `start` reach the window; the result depends on the seeds alone."""
    off = float(start)
    for _ in range(40):
        b = (books + np.float32(off)).astype(np.float32)
        sls = [classify(_tables(b, qq))["sl"] for qq in q]
        if lo <= min(sls) and max(sls) < hi:
            return np.float32(off)
        off = round(off * ((lo + hi) / 2.0 - 34.0) / ((min(sls) + max(sls)) / 2.0 - 34.0), 1)
    raise AssertionError("no offset puts every query's slack into [%d, %d)" % (lo, hi))


_cache = {}


def make_case(name, D=128, M=16, K=256, rows=ROWS, seed=SEED):
    """(books [M][K][D/M] f32, queries [nq][D] f32, codes [rows][M] u8).  Cached: callers must not write into the arrays."""
    key = (name, D, M, K, rows, seed)
    if key in _cache:
        return _cache[key]
    books, q, codes = _base(D, M, K, rows, seed)
    step = D // M
    if name == "constant":
        books = np.ascontiguousarray(np.repeat(books[:, :1], K, axis=1))
    elif name == "one_live":
        live = ONE_LIVE_M % M
        flat = np.repeat(books[:, :1], K, axis=1)
        flat[live] = books[live]
        books = np.ascontiguousarray(flat)
    elif name in SCALED:
        s = np.float32(SCALED[name])
        with np.errstate(all="ignore"):
            books = (books * s).astype(np.float32); q = (q * s).astype(np.float32)
    elif name == "shift3000":
        books = (books + _shift_for_window(books, q, 1000, 1024, 3000.0)).astype(np.float32)
    elif name == "shift1e4":
        books = (books + np.float32(1e4)).astype(np.float32)
    elif name == "dominant":
        books = books.copy(); q = q.copy()
        books[0] *= np.float32(1e6); q[:, :step] *= np.float32(1e6)
    elif name == "mixed":
        q0 = q[0].copy()
        with np.errstate(all="ignore"):
            q = np.stack([
                q0,                                                         # 0 ordinary
                books[:, MIXED_CODEWORD].reshape(-1),                       # 1 on a codeword of every sub-quantiser: bias 0
                q[2] * np.float32(1e4),                                     # 2 lazy on, a slack in the hundreds
                q[3] * np.float32(1e6),                                     # 3 slack >= 1024: lazy off on finite tables
                q[4] * np.float32(1e18),                                    # 4 the codewords are absorbed: range 0, sums finite
                q[5] * np.float32(2e19),                                    # 5 entries finite, every row sum +inf
                q[6],                                                       # 6 one NaN component
                np.full(D, -0.0, np.float32),                               # 7 every component -0.0
                q0,                                                         # 8 query 0 again: a group of one real query
            ]).astype(np.float32)
        q[6, 17 % D] = np.nan
    else:
        raise KeyError(name)
    out = (np.ascontiguousarray(books, dtype=np.float32), np.ascontiguousarray(q, dtype=np.float32), codes)
    for a in out:
        a.setflags(write=False)
    _cache[key] = out
    return out


def lut_of(orc, books, q):
    """the oracle's fp32 tables of one query, zero centroid"""
    return orc.lut(q, np.zeros(q.shape[0], np.float32), books)


def nan_free(q):
    """queries whose answers are checked: a NaN-bearing query must only leave the others of its batch alone"""
    return ~np.isnan(q).any(axis=1)


_oracle_cache = {}


def oracle_search(orc, key, books, q, codes, k):
    """orc.adc_search, computed once per (case key, k) and shared by the routes; callers must not write into the result"""
    ck = (key, k, q.shape[0])
    if ck not in _oracle_cache:
        with np.errstate(all="ignore"):
            d, i = orc.adc_search(q, books, codes, k)
        d.setflags(write=False); i.setflags(write=False)
        _oracle_cache[ck] = (d, i)
    return _oracle_cache[ck]


def tuning_default(name):
    """the default of a cvtmi_set_tuning key, as csrc/tuning.def states it"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cvt_amd", "csrc", "tuning.def")
    m = re.search(r"^TUNE\(%s,\s*([-0-9 <]+)," % re.escape(name), open(path).read(), flags=re.M)
    assert m, "no tuning key " + name
    expr = m.group(1).strip()
    if "<<" in expr:
        a, b = expr.split("<<")
        return int(a) << int(b)
    return int(expr)


@contextlib.contextmanager
def tuning(amd, **keys):
    """cvtmi_set_tuning for the block; every key goes back to its default from csrc/tuning.def, whatever happens inside"""
    try:
        for name, value in keys.items():
            amd.set_tuning(name, value)
        yield
    finally:
        for name in keys:
            amd.set_tuning(name, tuning_default(name))
