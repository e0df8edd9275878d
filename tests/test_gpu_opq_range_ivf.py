"""GPU: cvtmi_opq_range_search_ivf -- every entry of the nprobe nearest coarse lists whose score is under a radius (csrc/ivf_range.hip).

Every comparison is on lims, distance BITS, ids and video ids, through the host-pointer (numpy) and the device-pointer (torch)
entry.  Expected values never come from the library: per query the composed oracle of test_gpu_opq_ivf_search (oracle_scores: the
probe heap of IVFOPQ.cpp:238-260 replayed in numpy, orc.lut / orc.adc_scan per probed list) gives (score, insertion index) of
every entry of the probed lists; put into the order of the list-ordered copy (list id ascending, insertion order inside a list),
the entries with score < float32(radius) are the result.  Radii are taken from the oracle's scores of the batch: its minimum (no
hit: the comparison is strict), the next float above it, quantiles, +inf."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

from conftest import bits

from oracle import binding as ob
from test_gpu_opq_ivf_search import Case, get_case, oracle_scores

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
INF = np.float32(np.inf)
OK, EINVAL, ESPACE = 0, -1, -7
SPILL_DEFAULT = 4096


@pytest.fixture(scope="module")
def amd():
    import torch
    torch.cuda.is_available()
    import cvt_amd
    return cvt_amd


# ------------------------------------------------------------------------------------------ the oracle
def copy_order_scores(orc, case, q_rot, nprobe):
    """per query (scores, insertion indices) of every entry of its probed lists, in the order of the list-ordered copy"""
    out = []
    for f in range(q_rot.shape[0]):
        s, i = oracle_scores(orc, case, q_rot[f], nprobe)
        o = np.lexsort((i, case.lists[i]))
        out.append((s[o], i[o]))
    return out


_scored = {}


def scored(orc, name, nprobe, nq=24, seed=7):
    """copy_order_scores of the shared cases' standard batch, computed once"""
    key = (name, nprobe, nq, seed)
    if key not in _scored:
        case = get_case(orc, name)
        q = case.queries(nq, seed=seed)
        _scored[key] = (q, copy_order_scores(orc, case, orc.reorder(case.perm, q), nprobe))
    return _scored[key]


def expected(sc, radius, id_base=0, videos=None):
    """(lims, dist, ids, video) of a batch from its copy-order scores"""
    r = np.float32(radius)
    d, i = [], []
    with np.errstate(invalid="ignore"):
        for s, e in sc:
            keep = s < r
            d.append(s[keep]); i.append(e[keep])
    lims = np.concatenate([[0], np.cumsum([x.size for x in d])]).astype(np.int64)
    d = np.concatenate(d).astype(np.float32) if d else np.zeros(0, np.float32)
    i = np.concatenate(i).astype(np.int64) if i else np.zeros(0, np.int64)
    v = (i if videos is None else videos[i]).astype(np.int32)
    return lims, d, i + id_base, v


def batch_scores(sc):
    a = np.concatenate([s for s, _ in sc])
    return a[np.isfinite(a)]


def radii_of(sc):
    a = batch_scores(sc)
    lo = a.min()
    return [np.float32(-1), np.float32(0), lo, np.nextafter(lo, INF), np.float32(np.quantile(a, 0.001)), np.float32(np.quantile(a, 0.1)),
            np.float32(np.quantile(a, 0.5)), INF]


def run_both(idx, q, nprobe, radius, rotate=True):
    """(lims, dist, ids, video) through the host-pointer and the device-pointer entry"""
    import torch
    host = idx.range_search_ivf(q, nprobe, radius, rotate=rotate, want_video=True)
    dev = idx.range_search_ivf(torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda(), nprobe, radius, rotate=rotate, want_video=True)
    torch.cuda.synchronize()
    return host, tuple(t.cpu().numpy() for t in dev)


def same(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(got[2], want[2])
            and np.array_equal(got[3], want[3]))


def check(idx, q, nprobe, radius, want, rotate=True, what=""):
    for tag, got in zip(("host", "dev"), run_both(idx, q, nprobe, radius, rotate)):
        assert got[0].dtype == np.int64 and got[1].dtype == np.float32 and got[2].dtype == np.int64 and got[3].dtype == np.int32
        assert same(got, want), "%s %s nprobe=%d radius=%r: lims %s want %s" % (what, tag, nprobe, radius, got[0][:8], want[0][:8])


def video_ids(n):
    return ((np.arange(n, dtype=np.int64) * 7 + 3) % 1000).astype(np.int32)


# ------------------------------------------------------------------------------------------ 1 parity
@pytest.mark.parametrize("name", ["case1", "case3", "odd"])
def test_parity(amd, orc, name):
    case = get_case(orc, name)
    n = case.lists.size
    vids = video_ids(n)
    plain = case.index(amd)
    withv = amd.OpqIndex(case.coarse, case.books, perm=case.perm)
    withv.add_codes(case.codes, case.lists, vids)
    probes = [1, 3, 16] + ([case.coarseK + 5] if case.coarseK <= 128 else [])
    sizes = set()
    for nprobe in probes:
        q, sc = scored(orc, name, nprobe)
        q_rot = orc.reorder(case.perm, q)
        for radius in radii_of(sc):
            for rotate in (True, False):
                qq = q if rotate else q_rot
                check(plain, qq, nprobe, radius, expected(sc, radius), rotate, name)
                want = expected(sc, radius, videos=vids)
                check(withv, qq, nprobe, radius, want, rotate, name + " with video ids")
            sizes.update(np.diff(want[0]).tolist())
    print("%s: hits per query from %d to %d" % (name, min(sizes), max(sizes)))
    assert min(sizes) == 0 and max(sizes) > 1000                          # empty, small and multi-thousand results
    plain.close(); withv.close()


def test_odd_smallest_score_is_shared(amd, orc):
    """the strict comparison: a radius equal to the smallest score returns nothing, the next float above it every entry that holds it"""
    q, sc = scored(orc, "odd", 3)
    a = batch_scores(sc)
    lo = a.min()
    assert abs(float(lo) - 0.14278) < 1e-5 and int((a == lo).sum()) > 10
    idx = get_case(orc, "odd").index(amd)
    for got in run_both(idx, q, 3, lo):
        assert (got[0] == 0).all() and got[1].size == 0
    for got in run_both(idx, q, 3, np.nextafter(lo, INF)):
        assert got[0][-1] == int((a == lo).sum()) and (bits(got[1]) == bits(lo)).all()
    idx.close()


# ------------------------------------------------------------------------------------------ 2 both fill routes
def test_both_fill_routes(amd, orc):
    try:
        for name, nprobe in (("case1", 1), ("case1", 16), ("case3", 3)):
            case = get_case(orc, name)
            idx = case.index(amd)
            q, sc = scored(orc, name, nprobe)
            radius = np.float32(np.quantile(batch_scores(sc), 0.5))
            want = expected(sc, radius)
            for spill in (0, 1, 4, SPILL_DEFAULT, 1 << 30):
                amd.set_tuning("ivf_range_spill", spill)
                check(idx, q, nprobe, radius, want, what="%s spill=%d" % (name, spill))
                p = idx.last_range_plan()
                assert p["spill"] <= spill and (spill > 0) == (p["spill"] > 0), p
            if (name, nprobe) == ("case1", 1):                            # both routes inside one call
                amd.set_tuning("ivf_range_spill", 64)
                check(idx, q, nprobe, radius, want, what="case1 spill=64")
                p = idx.last_range_plan()
                per_query = np.diff(want[0])
                print("spill 64: %s, hits per query %d .. %d" % (p, per_query.min(), per_query.max()))
                assert p["spill"] == 64
                assert (per_query[per_query > 0] <= 64).any(), "a query whose parts all stay inside the capacity"
                assert (per_query > 64 * p["parts"]).any(), "a query with a part beyond the capacity"
            idx.close()
    finally:
        amd.set_tuning("ivf_range_spill", SPILL_DEFAULT)


# ------------------------------------------------------------------------------------------ 3 grid rules
def test_grid_rules(amd, orc):
    case = get_case(orc, "case1")
    idx = case.index(amd)
    q, sc = scored(orc, "case1", 3, nq=600, seed=17)
    radius = np.float32(np.quantile(batch_scores(sc[:24]), 0.5))
    want = expected(sc, radius)
    check(idx, q[:1], 3, radius, expected(sc[:1], radius), what="grid nq=1")
    p = idx.last_range_plan()
    print("nq=1: %s" % p)
    assert p["pieces"] > 1 and p["G"] == 1 and p["rule"] == 3, p             # the long list is cut, one list per workgroup
    check(idx, q[:24], 3, radius, expected(sc[:24], radius), what="grid nq=24")
    check(idx, q, 3, radius, want, what="grid nq=600")
    p = idx.last_range_plan()
    print("nq=600: %s" % p)
    assert p["pieces"] == 1 and p["G"] == 3 and p["parts"] == 1 and p["rule"] == 1, p
    try:
        amd.set_tuning("ivf_part_cap_mb", 1)                              # the spill area has to fit: fewer records per part
        amd.set_tuning("ivf_range_spill", 1 << 30)
        check(idx, q, 3, radius, want, what="grid rule 4")
        p = idx.last_range_plan()
        print("nq=600 under a 1 MB cap: %s" % p)
        assert p["rule"] == 4 and 0 < p["spill_bytes"] <= 1 << 20 and p["spill"] < 3 * case.longest(), p
        amd.set_tuning("ivf_part_cap_mb", 0)                              # no room at all: every part with a hit is walked twice
        check(idx, q, 3, radius, want, what="grid no spill area")
        assert idx.last_range_plan()["spill"] == 0
    finally:
        amd.set_tuning("ivf_part_cap_mb", 256)
        amd.set_tuning("ivf_range_spill", SPILL_DEFAULT)
    # nprobe 16 at 24 queries: groups of several lists, lists whole
    q16, sc16 = scored(orc, "case1", 16)
    check(idx, q16, 16, radius, expected(sc16, radius), what="grid groups")
    p = idx.last_range_plan()
    print("nq=24 nprobe=16: %s" % p)
    assert p["groups"] > 1 and (p["pieces"] == 1 or p["G"] == 1), p
    idx.close()


# ------------------------------------------------------------------------------------------ 4 capacity protocol
def raw_host(amd, idx, q, nprobe, radius, cap, lims, d, i, v, nq=None):
    def ptr(a):
        return C.c_void_p(0) if a is None else C.c_void_p(a.ctypes.data)
    q = np.ascontiguousarray(q, np.float32)
    return amd.lib().cvtmi_opq_range_search_ivf(idx.h, ptr(q), C.c_int64(q.shape[0] if nq is None else nq), C.c_int(1), C.c_int(nprobe), C.c_float(float(radius)),
                                                C.c_int64(cap), ptr(lims), ptr(d), ptr(i), ptr(v))


def raw_dev(amd, idx, q, nprobe, radius, cap, lims, d, i, v, nq=None):
    import torch

    def ptr(a):
        return C.c_void_p(0) if a is None else C.c_void_p(a.data_ptr())
    rc = amd.lib().cvtmi_opq_range_search_ivf_dev(idx.h, ptr(q), C.c_int64(q.shape[0] if nq is None else nq), C.c_int(1), C.c_int(nprobe), C.c_float(float(radius)),
                                                  C.c_int64(cap), ptr(lims), ptr(d), ptr(i), ptr(v), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def test_capacity_protocol(amd, orc):
    import torch
    case = get_case(orc, "case1")
    idx = case.index(amd)
    q, sc = scored(orc, "case1", 3)
    radius = np.float32(np.quantile(batch_scores(sc), 0.1))
    want = expected(sc, radius)
    total = int(want[0][-1])
    assert total > 100
    nq = q.shape[0]
    qd = torch.from_numpy(q).cuda()
    for cap, fits in ((total, True), (total - 1, False), (total + 7, True), (0, False)):
        room = max(cap, 1) + 3
        # host pointers
        lims = np.full(nq + 1, -5, np.int64)
        d = np.full(room, -3.0, np.float32); i = np.full(room, -9, np.int64); v = np.full(room, -4, np.int32)
        rc = raw_host(amd, idx, q, 3, radius, cap, lims, d, i, v)
        assert rc == (OK if fits else ESPACE), (cap, rc)
        assert np.array_equal(lims, want[0])
        if fits:
            assert same((lims, d[:total], i[:total], v[:total]), want)
            assert (d[total:] == -3.0).all() and (i[total:] == -9).all() and (v[total:] == -4).all()
        else:
            assert (d == -3.0).all() and (i == -9).all() and (v == -4).all()
        # device pointers: always OK, the fill is predicated on the device
        lims_t = torch.full((nq + 1,), -5, dtype=torch.int64, device="cuda")
        d_t = torch.full((room,), -3.0, dtype=torch.float32, device="cuda")
        i_t = torch.full((room,), -9, dtype=torch.int64, device="cuda")
        v_t = torch.full((room,), -4, dtype=torch.int32, device="cuda")
        assert raw_dev(amd, idx, qd, 3, radius, cap, lims_t, d_t, i_t, v_t) == OK
        lims, d, i, v = (t.cpu().numpy() for t in (lims_t, d_t, i_t, v_t))
        assert np.array_equal(lims, want[0])
        if fits:
            assert same((lims, d[:total], i[:total], v[:total]), want)
            assert (d[total:] == -3.0).all() and (i[total:] == -9).all() and (v[total:] == -4).all()
        else:
            assert (d == -3.0).all() and (i == -9).all() and (v == -4).all()
    # without a video array
    lims = np.zeros(nq + 1, np.int64); d = np.zeros(total, np.float32); i = np.zeros(total, np.int64)
    assert raw_host(amd, idx, q, 3, radius, total, lims, d, i, None) == OK
    assert np.array_equal(bits(d), bits(want[1])) and np.array_equal(i, want[2])
    # the count-only call: NULL arrays
    lims = np.full(nq + 1, -5, np.int64)
    assert raw_host(amd, idx, q, 3, radius, 0, lims, None, None, None) == OK and np.array_equal(lims, want[0])
    lims_t = torch.full((nq + 1,), -5, dtype=torch.int64, device="cuda")
    assert raw_dev(amd, idx, qd, 3, radius, 0, lims_t, None, None, None) == OK and np.array_equal(lims_t.cpu().numpy(), want[0])
    # the binding with the caller's arrays: raises when they are short
    out = (np.zeros(nq + 1, np.int64), np.zeros(total, np.float32), np.zeros(total, np.int64), np.zeros(total, np.int32))
    assert same(idx.range_search_ivf(q, 3, radius, out=out), want)
    short = (np.zeros(nq + 1, np.int64), np.zeros(total - 1, np.float32), np.zeros(total - 1, np.int64))
    with pytest.raises(amd.CvtmiError) as e:
        idx.range_search_ivf(q, 3, radius, out=short)
    assert e.value.code == ESPACE and np.array_equal(short[0], want[0])
    # nq == 0 writes lims[0] = 0 and nothing else
    lims = np.full(3, -5, np.int64)
    assert raw_host(amd, idx, q, 3, radius, 0, lims, None, None, None, nq=0) == OK and lims.tolist() == [0, -5, -5]
    lims_t = torch.full((3,), -5, dtype=torch.int64, device="cuda")
    assert raw_dev(amd, idx, qd, 3, radius, 0, lims_t, None, None, None, nq=0) == OK and lims_t.cpu().tolist() == [0, -5, -5]
    # argument checks on a live handle
    lims = np.zeros(nq + 1, np.int64)
    assert raw_host(amd, idx, q, 3, radius, 5, lims, None, i, None) == EINVAL
    assert raw_host(amd, idx, q, 3, radius, -1, lims, d, i, None) == EINVAL
    assert raw_host(amd, idx, q, 0, radius, 0, lims, None, None, None) == EINVAL
    idx.close()


# ------------------------------------------------------------------------------------------ 5 non-finite
def test_non_finite(amd, orc):
    base = get_case(orc, "case3")                                         # K = 200
    case = Case(32, 4, 200, 40, seed=9)
    case.perm, case.books, case.coarse = base.perm, base.books, base.coarse
    codes = base.codes[:1500].copy()
    planted = np.arange(3, codes.shape[0], 11)
    codes[planted, planted % 4] = 200 + (planted % 56).astype(np.uint8)   # code bytes >= K: +inf scores
    case.set_entries(base.lists[:1500], codes)
    idx = case.index(amd)
    q = case.queries(10, seed=12)
    q[4, 9] = np.inf
    q[2, 5] = np.nan
    q[7, :] = np.nan
    q_rot = orc.reorder(case.perm, q)
    for nprobe in (3, 40):
        sc = copy_order_scores(orc, case, q_rot, nprobe)
        a = batch_scores(sc)
        for radius in (np.float32(np.quantile(a, 0.3)), a.max(), INF):
            want = expected(sc, radius)
            per_query = np.diff(want[0])
            assert per_query[2] == 0 and per_query[4] == 0 and per_query[7] == 0 and per_query.sum() > 0   # the NaN and inf queries
            assert radius != INF or (per_query[[0, 1, 3, 5, 6, 8, 9]] > 0).all()                              # ... and their neighbours
            assert not np.isin(want[2], planted).any()
            check(idx, q, nprobe, radius, want, what="non-finite")
        every = expected(sc, INF)                                         # radius = +inf: every entry with a finite score
        finite = [int(np.isfinite(s).sum()) for s, _ in sc]
        assert np.diff(every[0]).tolist() == finite and sum(finite) < sum(s.size for s, _ in sc)
    for bad in (np.nan, -np.nan):
        with pytest.raises(amd.CvtmiError) as e:
            idx.range_search_ivf(q, 3, bad)
        assert e.value.code == EINVAL
    import torch
    with pytest.raises(amd.CvtmiError) as e:
        idx.range_search_ivf(torch.from_numpy(q).cuda(), 3, np.nan)
    assert e.value.code == EINVAL
    idx.close()


# ------------------------------------------------------------------------------------------ 6 two more checkers
def test_per_video_minimum_is_query_video(amd, orc):
    case = get_case(orc, "case1")
    n = case.lists.size
    vids = (np.arange(n) // 50).astype(np.int32)
    img_num = int(vids.max()) + 1
    idx = amd.OpqIndex(case.coarse, case.books, perm=case.perm)
    idx.add_codes(case.codes, case.lists, vids)
    q, sc = scored(orc, "case1", 3)
    ms = idx.query_video(q, 3, img_num)
    lims, d, i, v = idx.range_search_ivf(q, 3, 1.0, want_video=True)
    assert same((lims, d, i, v), expected(sc, 1.0, videos=vids))
    assert (ms < 1.0).any()
    for f in range(q.shape[0]):
        cell = np.full(img_num, 1.0, np.float32)
        np.minimum.at(cell, v[lims[f]:lims[f + 1]], d[lims[f]:lims[f + 1]])
        assert np.array_equal(bits(cell), bits(ms[f]))                    # videos without a hit hold 1.0
    idx.close()


def test_single_list_equals_exhaustive_search(amd, orc):
    case = Case(128, 16, 256, 1, seed=21)
    x = case.rows(5000)
    case.x_rot = orc.reorder(case.perm, x)
    case.coarse = case.x_rot[:1].copy() * np.float32(0.5)
    _, codes = orc.pq_encode(case.x_rot, case.coarse, case.books)
    idx = amd.OpqIndex(case.coarse, case.books, perm=case.perm)
    idx.add_codes(codes[:4000]); idx.add_codes(codes[4000:])
    q = case.queries(40, seed=2)
    d0, i0 = idx.search(q, 2048)
    radius = d0[:, 2047].min()                                            # below every query's 2048-th distance: the lists hold every hit
    dd, ii = [], []
    for f in range(q.shape[0]):
        keep = d0[f] < radius
        o = np.argsort(i0[f][keep], kind="stable")
        dd.append(d0[f][keep][o]); ii.append(i0[f][keep][o])
    lims = np.concatenate([[0], np.cumsum([x.size for x in dd])]).astype(np.int64)
    want = (lims, np.concatenate(dd), np.concatenate(ii), np.concatenate(ii).astype(np.int32))
    assert lims[-1] > 1000
    check(idx, q, 1, radius, want, what="coarseK == 1")
    check(idx, q, 4, radius, want, what="coarseK == 1, nprobe clamped")
    idx.close()


@pytest.mark.skipif(not ob.ref_available(), reason="oracle/_ref not built")
def test_live_reference_agrees(amd, orc):
    case = Case(32, 4, 256, 8, seed=5).encoded(orc, 160)
    raw = orc.reorder(np.argsort(case.perm).astype(np.int32), case.x_rot)   # rows whose permutation is x_rot
    ref = ob.RefOPQ(case.coarse, case.books, case.perm)
    try:
        ref.index([raw[e:e + 1] for e in range(raw.shape[0])])            # one video per entry
        q = case.queries(6, seed=3)
        ms = ref.query(q, 2, raw.shape[0])
    finally:
        ref.close()
    dd, ii = [], []
    for f in range(q.shape[0]):                                           # the reference's threshold test itself: cells under 1.0
        e = np.nonzero(ms[f] < 1.0)[0]
        o = np.lexsort((e, case.lists[e]))
        dd.append(ms[f][e][o]); ii.append(e[o].astype(np.int64))
    lims = np.concatenate([[0], np.cumsum([x.size for x in dd])]).astype(np.int64)
    want = (lims, np.concatenate(dd), np.concatenate(ii), np.concatenate(ii).astype(np.int32))
    assert lims[-1] > 0
    idx = case.index(amd)
    check(idx, q, 2, 1.0, want, what="live reference")
    idx.close()


# ------------------------------------------------------------------------------------------ 7 handle state
def test_handle_state(amd, orc):
    case = get_case(orc, "case3")
    n = case.lists.size
    q = case.queries(10, seed=8)
    q_rot = orc.reorder(case.perm, q)
    lists = case.lists.copy()
    lists[5::37] = -1                                                     # rows no list holds ...
    lists[11::41] = case.coarseK                                          # ... on either side of the range
    part = Case(32, 4, 200, 40, seed=3)
    part.perm, part.books, part.coarse = case.perm, case.books, case.coarse
    idx = amd.OpqIndex(case.coarse, case.books, perm=case.perm)
    idx.add_codes(case.codes[:1201], lists[:1201])
    part.set_entries(lists[:1201], case.codes[:1201])
    sc = copy_order_scores(orc, part, q_rot, 3)
    radius = np.float32(np.quantile(batch_scores(sc), 0.5))
    check(idx, q, 3, radius, expected(sc, radius), what="first block")
    idx.add_codes(case.codes[1201:], lists[1201:])                        # append at an odd count: ids continue
    part.set_entries(lists, case.codes)
    sc = copy_order_scores(orc, part, q_rot, 3)
    want = expected(sc, radius)
    assert want[2].max() >= 1201 and not np.isin(want[2], np.nonzero((lists < 0) | (lists >= case.coarseK))[0]).any()
    check(idx, q, 3, radius, want, what="after append")
    idx.set_id_base(10 ** 10)
    check(idx, q, 3, radius, expected(sc, radius, id_base=10 ** 10), what="id base")
    idx.set_id_base(0)
    sc_all = copy_order_scores(orc, part, q_rot, 45)                      # every list, the empty ones included
    assert (np.diff(part.list_off) == 0).any()
    check(idx, q, 45, INF, expected(sc_all, INF), what="every list")
    assert expected(sc_all, INF)[0][-1] == 10 * part.list_off[-1]
    idx.reset()
    for got in run_both(idx, q, 3, INF):
        assert (got[0] == 0).all() and got[0].size == 11 and got[1].size == 0
    idx.add_codes(case.codes[1000:1777], lists[1000:1777])
    part.set_entries(lists[1000:1777], case.codes[1000:1777])
    sc = copy_order_scores(orc, part, q_rot, 16)
    check(idx, q, 16, radius, expected(sc, radius), what="after reset")
    none = amd.OpqIndex(case.coarse, case.books, perm=case.perm)          # every entry outside the lists
    none.add_codes(case.codes[:500], np.full(500, -1, np.int32))
    for got in run_both(none, q, 3, INF):
        assert (got[0] == 0).all()
    idx.close(); none.close()


# ------------------------------------------------------------------------------------------ 8 concurrency
def test_concurrent_searches(amd, orc):
    case = get_case(orc, "case1")
    idx = case.index(amd)
    q, sc = scored(orc, "case1", 3, nq=600, seed=17)
    a = batch_scores(sc[:24])
    radii = [np.float32(np.quantile(a, t)) for t in (0.01, 0.1, 0.5, 0.9)]
    serial = [idx.range_search_ivf(q, 3, r, want_video=True) for r in radii]
    serial_topk = idx.search_ivf(q, 3, 100)
    got = [None] * 5
    errs = []

    def work(j):
        try:
            for _ in range(4):
                got[j] = idx.range_search_ivf(q, 3, radii[j], want_video=True) if j < 4 else idx.search_ivf(q, 3, 100)
        except Exception as e:   # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=work, args=(j,)) for j in range(5)]
    for t in ts: t.start()
    for t in ts: t.join()
    assert not errs, errs
    for j in range(4):
        assert same(got[j], serial[j])
    assert np.array_equal(bits(got[4][0]), bits(serial_topk[0])) and np.array_equal(got[4][1], serial_topk[1])
    assert same(serial[2], expected(sc, radii[2]))
    idx.close()


# ------------------------------------------------------------------------------------------ 9 one larger shape
def test_larger_shape(amd, orc):
    import torch
    from cvt_amd import synth
    D, M, K, L, n, nq, nprobe = 128, 16, 256, 1024, 100000, 1000, 8
    x = synth.sift_like(n, D, device="cuda")
    q = synth.sift_like(nq, D, seed=0xBEEF, device="cuda")
    perm = synth.random_permutation(D)
    sel = torch.randperm(n, generator=torch.Generator().manual_seed(5))[:L].cuda()
    probe = amd.OpqIndex(np.zeros((1, D), np.float32), np.zeros((M, K, D // M), np.float32), perm=perm)
    xr = probe.rotate(x)
    coarse = xr[sel].cpu().numpy()
    res = xr[:32768] - xr[sel[torch.randint(0, L, (32768,), generator=torch.Generator().manual_seed(6)).cuda()]]
    books = synth.train_books(res, M, K, iters=2)
    probe.close()
    idx = amd.OpqIndex(coarse, books, perm=perm)
    lists, codes = idx.encode(xr)
    idx.add_codes(codes, lists)
    case = Case(D, M, K, L, seed=0)
    case.perm, case.books, case.coarse = np.asarray(perm, np.int32), np.asarray(books, np.float32), coarse
    case.set_entries(lists.cpu().numpy(), codes.cpu().numpy())
    pick = np.linspace(0, nq - 1, 24).astype(int)
    qn = q.cpu().numpy()
    sc = copy_order_scores(orc, case, orc.reorder(case.perm, qn[pick]), nprobe)
    radius = np.float32(np.quantile(batch_scores(sc), 0.01))
    lims, d, i = idx.range_search_ivf(q, nprobe, radius)
    torch.cuda.synchronize()
    lims, d, i = lims.cpu().numpy(), d.cpu().numpy(), i.cpu().numpy()
    print("larger shape: %s, %d hits, per query %d .. %d" % (idx.last_range_plan(), lims[-1], np.diff(lims).min(), np.diff(lims).max()))
    want = expected(sc, radius)
    for j, f in enumerate(pick):
        a, b = want[0][j], want[0][j + 1]
        assert np.array_equal(bits(d[lims[f]:lims[f + 1]]), bits(want[1][a:b])) and np.array_equal(i[lims[f]:lims[f + 1]], want[2][a:b])
    dk, _ = idx.search_ivf(q, nprobe, 2048)                               # every query's count, where the top 2048 can tell it
    under = (dk.cpu().numpy() < radius).sum(axis=1)
    known = under < 2048
    assert known.sum() > nq // 2 and np.array_equal(np.diff(lims)[known], under[known])
    assert (i >= 0).all() and (i < n).all() and (d < radius).all()
    idx.close()


# ------------------------------------------------------------------------------------------ 10 host layers
def test_cli_radius(tmp_path, amd, orc, golden):
    """opq_search --nprobe 3 --radius R (IVFOPQ::RangeSearchProbe underneath) on the golden IVF model and data returns the ABI's hits."""
    exe = os.path.join(BIN, "opq_search")
    assert os.path.exists(exe), "host CLIs not built: __graft_entry__.build()"
    g = golden.opq["opq_ivf"]
    model = str(tmp_path / "model.bin")
    ob.write_opq_model(model, g["coarse"], g["books"], g["perm"])
    np.ascontiguousarray(g["db"], np.float32).tofile(str(tmp_path / "db.bin"))
    np.ascontiguousarray(g["queries"], np.float32).tofile(str(tmp_path / "q.bin"))
    idx = amd.OpqIndex(g["coarse"], g["books"], perm=g["perm"])
    lists, codes = idx.rotate_encode(g["db"])
    idx.add_codes(codes, lists)
    case = Case(32, 4, 256, 16, seed=0)                                   # the oracle, on the golden codes' own lists
    case.perm, case.books, case.coarse = g["perm"], g["books"], g["coarse"]
    case.set_entries(lists, codes)
    sc = copy_order_scores(orc, case, orc.reorder(case.perm, g["queries"]), 3)
    radius = np.float32(np.quantile(batch_scores(sc), 0.5))
    want = expected(sc, radius)
    check(idx, g["queries"], 3, radius, want, what="golden")
    r = subprocess.run([exe, model, "db.bin", "q.bin", "res.txt", "--nprobe", "3", "--radius", "%.9g" % radius], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = (tmp_path / "res.txt").read_text().splitlines()
    nq = g["queries"].shape[0]
    assert len(lines) == 2 * nq
    for f in range(nq):
        a, b = want[0][f], want[0][f + 1]
        head, ids_s = lines[2 * f].split(" ids:")
        head2, d_s = lines[2 * f + 1].split(" dists:")
        assert int(head) == f and int(head2) == f
        assert [int(t) for t in ids_s.split()] == want[2][a:b].tolist()
        assert np.array_equal(bits(np.array([float(t) for t in d_s.split()], np.float32)), bits(want[1][a:b]))   # %.9g round-trips fp32
    # --radius needs --nprobe
    r = subprocess.run([exe, model, "db.bin", "q.bin", "res2.txt", "--radius", "0.5"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "usage: opq_search" in r.stderr
    idx.close()
