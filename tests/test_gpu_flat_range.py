"""GPU: cvtmi_flat_range_search (csrc/flat_range.hip) and the layers above it.

Every comparison is exact.  Expectations never come from the code under test:
  fp32   orc.dist(metric, flavour, q, row) per pair, flavour 4 for IP and 8 for L2F (the choice test_gpu_flat_f32_bounds.py makes);
         the larger case takes orc.flat_search(k = n) re-sorted by row, which is the same numbers for NaN-free data;
  uint8  numpy int64 ((q - x) ** 2)[: D // 4 * 4].sum().
A row hits when distance < radius as real numbers: the expectation compares in float64, which holds every fp32 and int32 exactly.

Shapes (test_gpu_flat_remove.py's): n around the 64-lane wave, the 64-row block of the fp32 layout and the 256-row tile; fp32 at
D = 4, 32, 128 (blocked rows, queries in SGPRs) and 37 (row-major, queries in LDS), uint8 at D = 32 (norms), 48 (16-byte pieces, no
norms) and 5 (single bytes, tail dropped); "range_part_rows" = 256 puts 5 parts, the last of one row, into 1025 rows."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IP, L2F, L2U8 = 0, 1, 2
NS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
LAYOUTS = [(IP, 4), (IP, 32), (IP, 128), (IP, 37), (L2F, 4), (L2F, 32), (L2F, 128), (L2F, 37), (L2U8, 32), (L2U8, 48), (L2U8, 5)]
LABEL_MODES = ["implicit", "implicit_base", "explicit", "explicit_x3"]
NQS = [1, 5, 9, 33]
BASE = 10 ** 10
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
INF = float("inf")
CVTMI_OK, CVTMI_ESPACE = 0, -7
FORM = {(IP, 4): 1, (IP, 32): 1, (IP, 128): 1, (IP, 37): 0, (L2F, 4): 1, (L2F, 32): 1, (L2F, 128): 1, (L2F, 37): 0,
        (L2U8, 32): 4, (L2U8, 48): 3, (L2U8, 5): 2, (L2U8, 80): 3, (L2U8, 160): 4}


def want_qt(metric, nq):
    """queries per workgroup: fp32 1 or 4 (flat_qtile), uint8 the smallest of 1, 4, 8, 16 that holds the batch"""
    if metric == L2U8:
        return 1 if nq <= 1 else (4 if nq <= 4 else (8 if nq <= 8 else 16))
    return 4 if nq >= 4 else 1


@pytest.fixture(scope="module")
def amd():
    import torch
    torch.cuda.is_available()
    import cvt_amd
    return cvt_amd


def make_rows(metric, n, D, seed):
    """rows with exact duplicates in them: ties at every radius"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(n, D), dtype=np.uint8) if metric == L2U8 else rng.normal(size=(n, D)).astype(np.float32)
    for j in range(3, n, 7):
        x[j] = x[j % 3]
    return x


def make_queries(metric, D, seed, nq, rows=None):
    rng = np.random.default_rng(seed + 77)
    q = rng.integers(0, 256, size=(nq, D), dtype=np.uint8) if metric == L2U8 else rng.normal(size=(nq, D)).astype(np.float32)
    if rows is not None and len(rows):
        q[0] = rows[0]   # the duplicated row itself: its copies tie (L2: at distance 0)
    return q


def make_labels(mode, n, seed):
    """(labels to add with or None, id_base, the labels the searches report)"""
    if mode == "implicit":
        return None, 0, np.arange(n, dtype=np.int64)
    if mode == "implicit_base":
        return None, BASE, BASE + np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(seed + 5)
    lab = rng.choice(np.arange(-4 * n - 8, 4 * n + 8), size=n, replace=False).astype(np.int64)   # unsorted, negatives among them
    lab[::5] += 2 ** 33                                                                            # ... and labels >= 2^32
    if n >= 3:
        lab[n // 2] = I64_MIN
        lab[n - 1] = I64_MAX
    if mode == "explicit_x3" and n >= 9:
        lab[n // 3] = lab[2 * n // 3] = lab[1]   # one label on three rows
    return lab, 0, lab.copy()


def build(amd, metric, D, rows, labels=None, base=0, part_rows=0, spill=None):
    ix = amd.FlatIndex(metric, D)
    if base:
        ix.set_id_base(base)
    if part_rows:
        ix.set_param("range_part_rows", part_rows)
    if spill is not None:
        ix.set_param("range_spill", spill)
    if len(rows):
        ix.add(rows, labels)
    return ix


def dist_matrix(orc, metric, x, q):
    """E[query][row]: the distance cvtmi_flat_search reports for the pair, from the CPU oracle / numpy"""
    if metric == L2U8:
        d4 = x.shape[1] // 4 * 4
        xi, qi = x[:, :d4].astype(np.int64), q[:, :d4].astype(np.int64)
        return np.stack([((xi - one) ** 2).sum(axis=1) for one in qi]).astype(np.int32).reshape(len(q), len(x))
    flavour = 4 if metric == IP else 8
    return np.array([orc.dist(metric, flavour, one, r) for one in q for r in x], dtype=np.float32).reshape(len(q), len(x))


def expect(E, reported, radius):
    """(lims, distances, labels) of `distance < radius` over real numbers, hits of a query in ascending row order"""
    with np.errstate(invalid="ignore"):
        hit = E.astype(np.float64) < radius
    lims = np.concatenate([[0], np.cumsum(hit.sum(axis=1))]).astype(np.int64)
    return lims, E[hit], np.broadcast_to(reported, E.shape)[hit]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def search(ix, q, radius, dev=False):
    if not dev:
        return ix.range_search(q, radius)
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        lims, d, i = ix.range_search(torch.from_numpy(q).cuda(), radius)
    s.synchronize()
    return lims.cpu().numpy(), d.cpu().numpy(), i.cpu().numpy()


def check(ix, q, radius, E, reported, what, dev=False):
    elims, ed, ei = expect(E, reported, radius)
    lims, d, i = search(ix, q, radius, dev)
    what = (what, radius, dev)
    assert np.array_equal(lims, elims), what
    assert d.dtype == ed.dtype and np.array_equal(bits(d), bits(ed)), what
    assert np.array_equal(i, ei), what
    return int(elims[-1])


def radii(metric, E):
    """the radius edges of a case: a distance that occurs (strict: the row and its ties are out), the next value above it (they are
    in), the same two around a mid distance, 0, a negative value, +inf, -inf, and a radius under every distance"""
    fin = np.sort(E[np.isfinite(E.astype(np.float64))].ravel())
    occurs = [E[0, 0], fin[len(fin) // 2], fin[-1]]
    out = []
    for d in occurs:
        if metric == L2U8:
            out += [float(d), float(d) + 1.0, float(d) + 0.5]
        else:
            out += [float(d), float(np.nextafter(np.float32(d), np.float32(np.inf)))]
    out += [0.0, -1.5, INF, -INF]
    out.append(float(fin[0]) if metric == L2U8 else float(np.nextafter(np.float32(fin[0]), np.float32(-np.inf))))   # under every distance
    return out


# ---- 1. every layout at the row counts around wave, block and tile; label modes, batch sizes and entries rotate through the grid ----
@pytest.mark.parametrize("metric,D", LAYOUTS)
def test_shapes_and_radius_edges(amd, orc, metric, D):
    turn = LAYOUTS.index((metric, D))
    for n in NS:
        mode = LABEL_MODES[turn % 4]
        nq = NQS[(turn // 2) % 4]
        dev = turn % 3 == 2
        turn += 1
        rows = make_rows(metric, n, D, seed=n + D)
        q = make_queries(metric, D, n, nq, rows=rows)
        labels, base, reported = make_labels(mode, n, seed=n)
        E = dist_matrix(orc, metric, rows, q)
        ix = build(amd, metric, D, rows, labels, base)
        what = (metric, D, n, nq, mode)
        rs = radii(metric, E)
        for r in rs:
            total = check(ix, q, r, E, reported, what, dev=dev)
            plan = ix.last_range_plan()
            if total:
                assert plan["form"] == FORM[(metric, D)] and plan["qt"] == want_qt(metric, nq), (what, plan)
        assert check(ix, q, rs[-1], E, reported, what) == 0          # under every distance: all-zero lims
        assert check(ix, q, INF, E, reported, what) == nq * n        # (finite rows: everything)
        ix.close()


def test_every_batch_size_on_one_table(amd, orc):
    for metric, D in [(IP, 32), (L2F, 37), (L2U8, 32), (L2U8, 5)]:
        n = 257
        rows = make_rows(metric, n, D, seed=D)
        ix = build(amd, metric, D, rows)
        for nq in NQS:
            q = make_queries(metric, D, nq, nq, rows=rows)
            E = dist_matrix(orc, metric, rows, q)
            for r in radii(metric, E)[:4]:
                check(ix, q, r, E, np.arange(n, dtype=np.int64), (metric, D, nq), dev=nq == 9)
        ix.close()


# ---- 2. uint8 above 2^24: the radius is a double ----
def test_u8_radius_above_2_pow_24(amd):
    D, n = 512, 64
    rng = np.random.default_rng(24)
    rows = rng.integers(0, 256, size=(n, D), dtype=np.uint8)
    q = np.zeros((2, D), np.uint8)
    q[1] = rng.integers(0, 256, size=D)
    base_row = np.zeros(D, np.uint8)
    base_row[:258] = 255
    base_row[258:261] = (27, 6, 1)                 # 258 * 255^2 + 27^2 + 6^2 + 1 = 2^24
    for extra, at in ((0, 7), (1, 20), (2, 41), (1, 63)):
        rows[at] = base_row
        rows[at, 261:261 + extra] = 1              # 2^24 + extra
    E = dist_matrix(None, L2U8, rows, q)
    assert E[0, 7] == 2 ** 24 and E[0, 20] == 2 ** 24 + 1 and E[0, 41] == 2 ** 24 + 2
    ix = build(amd, L2U8, D, rows)
    reported = np.arange(n, dtype=np.int64)
    hits = {}
    for r in (2.0 ** 24, 2.0 ** 24 + 1, 2.0 ** 24 + 2, 2.0 ** 24 + 0.5, 2.0 ** 24 + 1.5, 2.0 ** 31, 2.0 ** 31 - 1, 1e300, INF):
        check(ix, q, r, E, reported, "2^24", dev=r == 2.0 ** 24 + 1)
        lims, d, i = ix.range_search(q[:1], r)
        hits[r] = set(i.tolist())
    assert 7 not in hits[2.0 ** 24] and 7 in hits[2.0 ** 24 + 1] and 20 not in hits[2.0 ** 24 + 1] and 63 not in hits[2.0 ** 24 + 1]
    assert {7, 20, 63} <= hits[2.0 ** 24 + 2] and 41 not in hits[2.0 ** 24 + 2]
    assert ix.last_range_plan()["form"] == 4
    ix.close()


# ---- 3. non-finite values, fp32 ----
@pytest.mark.parametrize("metric,D", [(IP, 32), (L2F, 32), (IP, 37), (L2F, 37), (L2F, 4)])
def test_non_finite(amd, orc, metric, D):
    n, nq = 300, 5
    rows = make_rows(metric, n, D, seed=D)
    q = make_queries(metric, D, 1, nq, rows=rows)
    q[:, 1] = np.abs(q[:, 1]) + 0.5
    rows[5, 2] = np.nan          # a NaN row never hits
    rows[70, 0] = np.nan
    rows[9, 1] = np.inf          # L2: distance +inf, absent even at radius +inf.  IP: 1 - (+inf) = -inf, present at every radius above -inf
    rows[257, 1] = np.inf
    q[2, :] = np.nan             # a NaN query has no hits
    E = dist_matrix(orc, metric, rows, q)
    assert np.isnan(E[:, 5]).all() and np.isnan(E[2]).all()
    assert (E[[0, 1, 3, 4]][:, [9, 257]] == (-np.inf if metric == IP else np.inf)).all()
    ix = build(amd, metric, D, rows)
    reported = np.arange(n, dtype=np.int64)
    for r in (INF, 1e30, 0.0, -1e30, -3.4028234663852886e38, -1e300, -INF, float(E[0, 1])):
        check(ix, q, r, E, reported, (metric, D, "non-finite"), dev=r == 0.0)
    lims, d, i = ix.range_search(q, INF)
    per_query = np.diff(lims)
    assert per_query[2] == 0
    assert not np.isin(i, [5, 70]).any()
    assert np.isin(9, i[:lims[1]]) == (metric == IP) and np.isin(257, i[:lims[1]]) == (metric == IP)
    if metric == IP:
        lims, d, i = ix.range_search(q, -1e300)          # only the -inf distances are below it
        assert np.array_equal(np.diff(lims), [2, 2, 0, 2, 2]) and np.isneginf(d).all()
    ix.close()


# ---- 4. part and spill seams ----
HUGE = 2 ** 40


# (uint8 80 and 160: rows longer than one step of the scan's read-ahead, four 16-byte pieces -- 5 pieces without norms, 10 with them)
@pytest.mark.parametrize("metric,D", [(IP, 32), (L2F, 128), (L2F, 37), (L2U8, 32), (L2U8, 48), (L2U8, 5), (L2U8, 80), (L2U8, 160)])
def test_part_and_spill_seams(amd, orc, metric, D):
    n, nq = 1025, 9
    rows = make_rows(metric, n, D, seed=3 * D)
    q = make_queries(metric, D, 9, nq, rows=rows)
    labels, base, reported = make_labels("explicit_x3", n, seed=11)
    E = dist_matrix(orc, metric, rows, q)
    mid = float(np.sort(E.ravel())[E.size // 3])
    few = float(np.unique(E)[40])                # 40 distinct distances under it: some parts hold a few hits, most none
    results = {}
    for spill, want_c in ((0, 0), (1, 1), (7, 7), (None, 256), (HUGE, 256)):   # the default 512 and the huge value are cut to the rows of a part
        ix = build(amd, metric, D, rows, labels, base, part_rows=256, spill=spill)
        for r in (INF, mid, few):
            check(ix, q, r, E, reported, (metric, D, "spill", spill), dev=spill == 1)
            plan = ix.last_range_plan()
            assert plan["parts"] == 5 and plan["rows_per_part"] == 256 and plan["spill"] == want_c, plan
            assert plan["spill_bytes"] == nq * 5 * want_c * 8 and plan["qt"] == want_qt(metric, nq) and plan["form"] == FORM[(metric, D)], plan
            results.setdefault(r, []).append(ix.range_search(q, r))
        ix.close()
    for r, got in results.items():
        for other in got[1:]:
            assert all(np.array_equal(bits(a) if a.dtype != np.int64 else a, bits(b) if b.dtype != np.int64 else b) for a, b in zip(got[0], other)), r


def test_part_rows_round_up_to_tiles(amd):
    rows = make_rows(L2F, 1025, 32, seed=1)
    ix = build(amd, L2F, 32, rows, part_rows=300)
    ix.range_search(rows[:4], 1.0)
    plan = ix.last_range_plan()
    assert plan["rows_per_part"] == 512 and plan["parts"] == 3, plan
    ix.close()


# ---- 5. one larger case for the default plan ----
@pytest.fixture(scope="module")
def large(orc):
    n, D, nq = 70000, 32, 9
    out = {}
    for metric in (IP, L2U8):
        rows = make_rows(metric, n, D, seed=70 + metric)
        q = make_queries(metric, D, 70, nq, rows=rows)
        if metric == IP:
            od, _, oi = orc.flat_search(IP, rows, q, n, flavour=4)
            E = np.empty((nq, n), np.float32)
            for f in range(nq):
                assert np.array_equal(np.sort(oi[f]), np.arange(n))
                E[f, oi[f]] = od[f]
        else:
            E = dist_matrix(None, L2U8, rows, q)
        out[metric] = (rows, q, E)
    return out


@pytest.mark.parametrize("metric", [IP, L2U8])
def test_larger_table_default_plan(amd, large, metric):
    rows, q, E = large[metric]
    n, D = rows.shape
    ix = build(amd, metric, D, rows, None, BASE)
    reported = BASE + np.arange(n, dtype=np.int64)
    assert check(ix, q, INF, E, reported, (metric, "large"), dev=True) == 9 * n
    plan = ix.last_range_plan()
    assert plan["parts"] > 1 and plan["qt"] == want_qt(metric, 9) and plan["spill"] == 512 and plan["parts"] * plan["rows_per_part"] >= n, plan
    r50 = float(np.sort(E[1])[50])             # 50 hits for query 1, about as many for the others; query 0 adds the copies of row 0
    total = check(ix, q, r50, E, reported, (metric, "large"))
    assert 50 <= total <= 9 * 5000, total
    check(ix, q, r50, E, reported, (metric, "large"), dev=True)
    ix.close()


# ---- 6. capacity ----
def raw(amd, ix, q, nq, radius, cap, lims, d, i, dev=False):
    from cvt_amd.capi import _ptr, _stream
    lib = amd.lib()
    args = (ix.h, _ptr(q), C.c_int64(nq), C.c_double(radius), C.c_int64(cap), _ptr(lims), _ptr(d), _ptr(i))
    if dev:
        return lib.cvtmi_flat_range_search_dev(*args, _stream())
    return lib.cvtmi_flat_range_search(*args)


@pytest.mark.parametrize("metric,D", [(L2F, 32), (L2U8, 48)])
def test_capacity(amd, orc, metric, D):
    import torch
    from cvt_amd.capi import CvtmiError
    n, nq = 700, 5
    rows = make_rows(metric, n, D, seed=D)
    q = make_queries(metric, D, 3, nq, rows=rows)
    E = dist_matrix(orc, metric, rows, q)
    r = float(np.sort(E.ravel())[333])
    reported = np.arange(n, dtype=np.int64)
    elims, ed, ei = expect(E, reported, r)
    total = int(elims[-1])
    assert total > 100
    ddt = np.int32 if metric == L2U8 else np.float32
    ix = build(amd, metric, D, rows, part_rows=256, spill=3)
    # count only
    lims = np.full(nq + 1, -5, np.int64)
    assert raw(amd, ix, q, nq, r, 0, lims, None, None) == CVTMI_OK and np.array_equal(lims, elims)
    assert ix.last_range_plan()["spill"] == 0
    # exactly enough room
    lims = np.full(nq + 1, -5, np.int64)
    d = np.full(total, 77, ddt); i = np.full(total, -77, np.int64)
    ix.range_search(q, r, out=(lims, d, i))
    assert np.array_equal(lims, elims) and np.array_equal(bits(d), bits(ed)) and np.array_equal(i, ei)
    # one short: CVTMI_ESPACE, arrays untouched, lims exact
    lims = np.full(nq + 1, -5, np.int64)
    d = np.full(total - 1, 77, ddt); i = np.full(total - 1, -77, np.int64)
    with pytest.raises(CvtmiError) as err:
        ix.range_search(q, r, out=(lims, d, i))
    assert err.value.code == CVTMI_ESPACE
    assert np.array_equal(lims, elims) and (d == 77).all() and (i == -77).all()
    # the device entry never waits: too small a cap returns CVTMI_OK, leaves the arrays alone and reports lims[nq] > cap
    qd = torch.from_numpy(q).cuda()
    tdt = torch.int32 if metric == L2U8 else torch.float32
    for cap in (total - 1, 1):
        lims_d = torch.full((nq + 1,), -5, dtype=torch.int64, device="cuda")
        d_d = torch.full((cap,), 77, dtype=tdt, device="cuda"); i_d = torch.full((cap,), -77, dtype=torch.int64, device="cuda")
        ix.range_search(qd, r, out=(lims_d, d_d, i_d))
        torch.cuda.synchronize()
        assert np.array_equal(lims_d.cpu().numpy(), elims) and int(lims_d[-1]) > cap
        assert bool((d_d == 77).all()) and bool((i_d == -77).all())
    lims_d = torch.full((nq + 1,), -5, dtype=torch.int64, device="cuda")
    d_d = torch.full((total + 3,), 77, dtype=tdt, device="cuda"); i_d = torch.full((total + 3,), -77, dtype=torch.int64, device="cuda")
    ix.range_search(qd, r, out=(lims_d, d_d, i_d))
    torch.cuda.synchronize()
    assert np.array_equal(lims_d.cpu().numpy(), elims) and np.array_equal(bits(d_d[:total].cpu().numpy()), bits(ed))
    assert np.array_equal(i_d[:total].cpu().numpy(), ei) and bool((d_d[total:] == 77).all()) and bool((i_d[total:] == -77).all())
    # device count-only
    lims_d = torch.full((nq + 1,), -5, dtype=torch.int64, device="cuda")
    assert raw(amd, ix, qd, nq, r, 0, lims_d, None, None, dev=True) == CVTMI_OK
    torch.cuda.synchronize()
    assert np.array_equal(lims_d.cpu().numpy(), elims)
    # nq == 0: lims[0] = 0 and nothing else
    lims = np.full(3, -5, np.int64)
    assert raw(amd, ix, q, 0, r, 4, lims, d, i) == CVTMI_OK and lims.tolist() == [0, -5, -5] and (d == 77).all()
    lims_d = torch.full((3,), -5, dtype=torch.int64, device="cuda")
    assert raw(amd, ix, qd, 0, r, 1, lims_d, d_d, i_d, dev=True) == CVTMI_OK
    torch.cuda.synchronize()
    assert lims_d.cpu().tolist() == [0, -5, -5]
    ix.close()
    # an empty index: all-zero lims, arrays untouched
    empty = amd.FlatIndex(metric, D)
    lims = np.full(nq + 1, -5, np.int64)
    assert raw(amd, empty, q, nq, INF, d.shape[0], lims, d, i) == CVTMI_OK and not lims.any() and (d == 77).all() and (i == -77).all()
    lims_d = torch.full((nq + 1,), -5, dtype=torch.int64, device="cuda")
    assert raw(amd, empty, qd, nq, INF, 1, lims_d, d_d, i_d, dev=True) == CVTMI_OK
    torch.cuda.synchronize()
    assert not lims_d.cpu().numpy().any()
    got = empty.range_search(q, INF)
    assert not got[0].any() and got[1].shape == (0,) and got[2].shape == (0,)
    empty.close()


# ---- 7. consistency with the top-k search ----
@pytest.mark.parametrize("metric,D", [(IP, 128), (L2F, 37), (L2U8, 32)])
def test_consistent_with_flat_search(amd, metric, D):
    n, nq, k = 1025, 33, 10
    rows = make_rows(metric, n, D, seed=D + 1)
    q = make_queries(metric, D, 4, nq, rows=rows)
    ix = build(amd, metric, D, rows, None, BASE)
    sd, si = ix.search(q, k)
    r = float(np.sort(sd[:, 4])[nq // 2])      # about half of the queries have fewer than 5 rows under it
    lims, d, i = ix.range_search(q, r)
    compared = 0
    for f in range(nq):
        under = sd[f].astype(np.float64) < r
        if under.sum() >= k:
            continue
        order = np.argsort(si[f][under], kind="stable")
        assert np.array_equal(i[lims[f]:lims[f + 1]], si[f][under][order]), f
        assert np.array_equal(bits(d[lims[f]:lims[f + 1]]), bits(sd[f][under][order])), f
        compared += 1
    assert compared >= nq // 2
    ix.close()


# ---- 8. after remove_labels and a further add ----
@pytest.mark.parametrize("metric,D", [(L2F, 128), (IP, 37), (L2U8, 32), (L2U8, 5)])
def test_after_remove_and_add(amd, orc, metric, D):
    n, nq = 700, 9
    rows = make_rows(metric, n, D, seed=D)
    q = make_queries(metric, D, 6, nq, rows=rows)
    rng = np.random.default_rng(D)
    ix = build(amd, metric, D, rows, None, BASE, part_rows=256)
    reported = BASE + np.arange(n, dtype=np.int64)
    keep = rng.random(n) >= 0.4
    assert ix.remove_labels(reported[~keep]) == int((~keep).sum())
    more = make_rows(metric, 333, D, seed=D + 9)
    lab = 5 * BASE + np.arange(333, dtype=np.int64)
    ix.add(more, lab)
    rows2, rep2 = np.concatenate([rows[keep], more]), np.concatenate([reported[keep], lab])
    fresh = build(amd, metric, D, rows2, rep2)
    E = dist_matrix(orc, metric, rows2, q)
    for r in (INF, float(np.sort(E.ravel())[E.size // 4])):
        a, b = ix.range_search(q, r), fresh.range_search(q, r)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])
        check(ix, q, r, E, rep2, (metric, D, "removed + added"))
    ix.close(); fresh.close()


# ---- 9. four threads on one handle ----
@pytest.mark.parametrize("metric,D", [(L2F, 32), (L2U8, 32)])
def test_four_threads_on_one_handle(amd, orc, metric, D):
    n, nq = 1025, 9
    rows = make_rows(metric, n, D, seed=D + 2)
    q = make_queries(metric, D, 8, nq, rows=rows)
    E = dist_matrix(orc, metric, rows, q)
    r = float(np.sort(E.ravel())[E.size // 5])
    ix = build(amd, metric, D, rows, part_rows=256, spill=5)
    elims, ed, ei = expect(E, np.arange(n, dtype=np.int64), r)
    got, errors = [None] * 4, []

    def work(t):
        try:
            res = []
            for _ in range(6):
                res.append(ix.range_search(q, r))
                ix.search(q, 10)                       # ... side by side with top-k searches
            got[t] = res
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for res in got:
        for lims, d, i in res:
            assert np.array_equal(lims, elims) and np.array_equal(bits(d), bits(ed)) and np.array_equal(i, ei)
    ix.close()


# ---- 10. the host mirror ----
def test_bruteforce_mirror_search_range():
    exe = os.path.join(ROOT, "cvt_amd", "bin", "bf_range_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.stdout, r.stderr)
