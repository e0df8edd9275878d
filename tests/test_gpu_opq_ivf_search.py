"""GPU: cvtmi_opq_search_ivf -- the k nearest entries among the nprobe nearest coarse lists (csrc/ivf_search.hip).

Every comparison is on distance BITS and ids, through host pointers (numpy) and device pointers (torch) unless a test says
otherwise.  Expected values never come from the library:

  composed oracle   per query the probe heap of IVFOPQ.cpp:238-260 replayed in numpy float32 (sequential d += t * t over
                    the dimensions, then the nprobe smallest (d, list)), and per probed list orc.lut / orc.adc_scan over
                    the list's entries; orc.topk_pairs of all (score, id) pairs gives the list.  It is computed once per
                    (data, queries, nprobe) for k = 2048: the k smallest pairs of a set are the first k of its 2048 smallest.
  cross-check       orc.query_video with one video per entry (video id = insertion index, img_num = n): on data whose scores
                    all stay below 1.0, match_score[q][e] < 1.0 holds exactly for the entries of the probed lists and is
                    their score.  Where oracle/_ref is built the reference itself answers one small case the same way.

Data: rows are drawn around a few centres with unequal weights (x 0.03, so that every score stays below 1.0) and the centroids are
rows of them, a few repeated, so the lists come out long, short and (behind a repeated centroid, which never wins the
first-minimum rule) empty."""
import os
import subprocess
import threading

import numpy as np
import pytest

from conftest import bits

from oracle import binding as ob

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
KMAX = 2048
INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def amd():
    import torch
    torch.cuda.is_available()
    import cvt_amd
    return cvt_amd


# ------------------------------------------------------------------------------------------ data
class Case:
    """A model (coarse, books, permutation) and n entries (list ids, codes) with their list-ordered view."""

    def __init__(self, D, M, K, coarseK, seed, scale=0.03):
        self.D, self.M, self.K, self.coarseK = D, M, K, coarseK
        self.rng = np.random.default_rng(seed)
        self.scale = scale
        self.perm = self.rng.permutation(D).astype(np.int32)
        self.books = (self.rng.normal(size=(M, K, D // M)) * scale).astype(np.float32)
        self.coarse = None
        self.lists = np.zeros(0, np.int32)
        self.codes = np.zeros((0, M), np.uint8)

    def rows(self, n, centres=12):
        c = self.rng.normal(size=(centres, self.D)) * self.scale
        w = 1.0 / np.arange(1, centres + 1) ** 1.5
        pick = self.rng.choice(centres, size=n, p=w / w.sum())
        self.centre_of_row = pick
        return (c[pick] * 0.7 + self.rng.normal(size=(n, self.D)) * self.scale * 0.7).astype(np.float32)

    def encoded(self, orc, n):
        """n rows through the oracle's encoder; centroids = rows drawn with replacement, each from a centre chosen uniformly: a centre
        that holds many rows gets no more centroids than one that holds few, so its lists are long"""
        x = self.rows(n)
        self.x_rot = orc.reorder(self.perm, x)
        centres = self.centre_of_row.max() + 1
        sel = [self.rng.choice(np.nonzero(self.centre_of_row == c)[0]) for c in self.rng.integers(0, centres, size=self.coarseK)]
        self.coarse = self.x_rot[np.array(sel)].copy()
        for j in range(7, self.coarseK, 13):                              # a repeated centroid: the later copy never wins, its list stays empty
            self.coarse[j] = self.coarse[j - 5]
        lists, codes = orc.pq_encode(self.x_rot, self.coarse, self.books)
        self.set_entries(lists, codes)
        return self

    def set_entries(self, lists, codes):
        self.lists = np.ascontiguousarray(lists, np.int32)
        self.codes = np.ascontiguousarray(codes, np.uint8)
        ok = (self.lists >= 0) & (self.lists < self.coarseK)
        idx = np.nonzero(ok)[0]
        order = idx[np.argsort(self.lists[idx], kind="stable")]           # list order, insertion order inside a list
        self.csr_entry = order
        self.list_off = np.concatenate([[0], np.cumsum(np.bincount(self.lists[idx], minlength=self.coarseK))]).astype(np.int64)

    def list_rows(self, l):
        return self.csr_entry[self.list_off[l]:self.list_off[l + 1]]

    def longest(self):
        return int(np.diff(self.list_off).max()) if self.coarseK else 0

    def index(self, amd, id_base=0):
        idx = amd.OpqIndex(self.coarse, self.books, perm=self.perm)
        if self.lists.size:
            idx.add_codes(self.codes, self.lists)
        if id_base:
            idx.set_id_base(id_base)
        return idx

    def queries(self, nq, seed=1):
        """RAW queries (before the permutation): rows of the same distribution"""
        rng, self.rng = self.rng, np.random.default_rng(seed)
        q = self.rows(nq)
        self.rng = rng
        return q


def probe_lists(q_rot, coarse, nprobe):
    """IVFOPQ.cpp:238-260: the nprobe smallest (sequential fp32 distance, list) pairs; a NaN never replaces the heap top, so a
    frame holding one keeps the first nprobe lists."""
    if np.isnan(q_rot).any():
        return np.arange(nprobe)
    acc = np.zeros(coarse.shape[0], np.float32)
    with np.errstate(all="ignore"):
        for d in range(coarse.shape[1]):
            t = np.float32(q_rot[d]) - coarse[:, d]
            acc = acc + t * t
    return np.lexsort((np.arange(coarse.shape[0]), acc))[:nprobe]


def lut256(orc, q_rot, centroid, books):
    lut = orc.lut(q_rot, centroid, books)                                 # [M][K]
    if lut.shape[1] < 256:                                               # code bytes >= K score +inf (the kernel's table is 256 wide)
        lut = np.concatenate([lut, np.full((lut.shape[0], 256 - lut.shape[1]), INF, np.float32)], axis=1)
    return np.ascontiguousarray(lut)


def oracle_scores(orc, case, q_rot, nprobe):
    """(scores, insertion indices) of every entry of the probed lists of one rotated query"""
    nprobe = min(nprobe, case.coarseK)
    sc, ids = [np.zeros(0, np.float32)], [np.zeros(0, np.int64)]
    with np.errstate(all="ignore"):
        for l in probe_lists(q_rot, case.coarse, nprobe):
            rows = case.list_rows(l)
            if rows.size:
                sc.append(orc.adc_scan(lut256(orc, q_rot, case.coarse[l], case.books), case.codes[rows]))
                ids.append(rows.astype(np.int64))
    return np.concatenate(sc), np.concatenate(ids)


def oracle_search(orc, case, q_raw, nprobe, rotate=True, id_base=0):
    """per query the (up to) KMAX smallest (score, id) pairs: list of (d, i)"""
    q_rot = orc.reorder(case.perm, q_raw) if rotate else np.ascontiguousarray(q_raw, np.float32)
    out = []
    for f in range(q_rot.shape[0]):
        s, i = oracle_scores(orc, case, q_rot[f], nprobe)
        if np.isnan(s).any():
            out.append((s, i + id_base))                                  # a NaN query: the candidate set, unordered
        else:
            out.append(orc.topk_pairs(s, KMAX, i + id_base))
    return out


def padded(exp, k):
    d = np.full((len(exp), k), INF, np.float32)
    i = np.full((len(exp), k), -1, np.int64)
    for f, (ed, ei) in enumerate(exp):
        m = min(k, ed.size)
        d[f, :m] = ed[:m]; i[f, :m] = ei[:m]
    return d, i


def run_both(idx, q, nprobe, k, rotate=True):
    """(distances, ids) through the host-pointer and the device-pointer entry"""
    import torch
    dh, ih = idx.search_ivf(q, nprobe, k, rotate=rotate)
    dd, id_ = idx.search_ivf(torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda(), nprobe, k, rotate=rotate)
    torch.cuda.synchronize()
    return (dh, ih), (dd.cpu().numpy(), id_.cpu().numpy())


def check(idx, q, nprobe, k, exp, rotate=True, nan_rows=(), what=""):
    ed, ei = padded(exp, k)
    keep = np.ones(len(exp), bool)
    keep[list(nan_rows)] = False
    for tag, (d, i) in zip(("host", "dev"), run_both(idx, q, nprobe, k, rotate)):
        bad = np.nonzero(keep & ((bits(d) != bits(ed)).any(axis=1) | (i != ei).any(axis=1)))[0]
        assert bad.size == 0, "%s %s nprobe=%d k=%d: %d queries differ, first %d: got %s / %s want %s / %s" % (
            what, tag, nprobe, k, bad.size, bad[0], d[bad[0]][:6], i[bad[0]][:6], ed[bad[0]][:6], ei[bad[0]][:6])
        for f in nan_rows:                                                # the rule cvtmi_opq_search has: NaN distances, distinct candidates
            cand = exp[f][1]
            m = min(k, cand.size)
            assert np.isnan(d[f, :m]).all() and np.array_equal(bits(d[f, m:]), bits(np.full(k - m, INF)))
            assert len(set(i[f, :m].tolist())) == m and set(i[f, :m].tolist()) <= set(cand.tolist()) and (i[f, m:] == -1).all()


SHAPES = {   # name: D, M, K, coarseK, n
    "case1": (128, 16, 256, 64, 20000),
    "case2": (64, 8, 256, 200, 6000),
    "case3": (32, 4, 200, 40, 3000),
    "odd": (96, 2, 17, 3, 1500),
    "wide": (128, 16, 256, 100, 8000),
}
_cases = {}


def get_case(orc, name):
    if name not in _cases:
        D, M, K, coarseK, n = SHAPES[name]
        _cases[name] = Case(D, M, K, coarseK, seed=100 + len(name) + D).encoded(orc, n)
    return _cases[name]


# ------------------------------------------------------------------------------------------ 1 parity
@pytest.mark.parametrize("name", list(SHAPES))
def test_seeded_parity(amd, orc, name):
    case = get_case(orc, name)
    if case.coarseK > 12:
        assert (np.diff(case.list_off) == 0).any(), "the data should hold empty lists"
    if name == "case1":
        assert case.longest() > 1024, "the data should hold a list of more than one piece"
    print("%s: longest list %d rows, %d empty lists" % (name, case.longest(), int((np.diff(case.list_off) == 0).sum())))
    idx = case.index(amd)
    q = case.queries(24, seed=7)
    probes = [1, 3, 16] + ([case.coarseK + 5] if case.coarseK <= 128 else [])
    for rotate in (True, False):
        qq = q if rotate else orc.reorder(case.perm, q)
        for nprobe in probes:
            exp = oracle_search(orc, case, qq, nprobe, rotate=rotate)
            for k in (1, 10, 100, 128, 129, 1000, 2048):
                check(idx, qq, nprobe, k, exp, rotate=rotate, what=name)
    idx.close()


# ------------------------------------------------------------------------------------------ 2 two checkers
def video_crosscheck(orc, case, q_rot, nprobe):
    n = case.lists.size
    ms = orc.query_video(q_rot, case.coarse, case.books, nprobe, case.list_off, case.codes[case.csr_entry], case.csr_entry.astype(np.int32), n)
    return ms


@pytest.mark.parametrize("name,nprobe,k", [("case1", 5, 100), ("case3", 3, 10)])
def test_two_checkers_agree(amd, orc, name, nprobe, k):
    case = get_case(orc, name)
    n = case.lists.size
    q = case.queries(16, seed=11)
    q_rot = orc.reorder(case.perm, q)
    # every score of the data stays below 1.0: seen on the run that probes everything
    ms_all = video_crosscheck(orc, case, q_rot, case.coarseK)
    kept = np.zeros(n, bool); kept[case.csr_entry] = True
    assert ms_all[:, kept].max() < 1.0, ms_all[:, kept].max()
    ms = video_crosscheck(orc, case, q_rot, nprobe)
    exp2 = []
    for f in range(q.shape[0]):
        e = np.nonzero(ms[f] < 1.0)[0]
        exp2.append(orc.topk_pairs(ms[f][e], KMAX, e.astype(np.int64)))
    exp1 = oracle_search(orc, case, q, nprobe)
    for (d1, i1), (d2, i2) in zip(exp1, exp2):                           # the two checkers agree with each other ...
        assert np.array_equal(bits(d1), bits(d2)) and np.array_equal(i1, i2)
    idx = case.index(amd)
    check(idx, q, nprobe, k, exp2, what=name + " cross-check")           # ... and the library with them
    # the library's own per-video query on the same handle: min(dist, 1.0) of the returned entries are its cells
    lib_ms = idx.query_video(q, nprobe, n)
    assert np.array_equal(bits(lib_ms), bits(ms))
    d, i = idx.search_ivf(q, nprobe, k)
    for f in range(q.shape[0]):
        real = i[f] >= 0
        assert np.array_equal(bits(np.minimum(d[f][real], np.float32(1.0))), bits(lib_ms[f][i[f][real]]))
    idx.close()


@pytest.mark.skipif(not ob.ref_available(), reason="oracle/_ref not built")
def test_live_reference_agrees(amd, orc):
    case = Case(32, 4, 256, 8, seed=5).encoded(orc, 160)
    raw = orc.reorder(np.argsort(case.perm).astype(np.int32), case.x_rot)   # rows whose permutation is x_rot
    assert np.array_equal(orc.reorder(case.perm, raw), case.x_rot)
    ref = ob.RefOPQ(case.coarse, case.books, case.perm)
    try:
        ref.index([raw[e:e + 1] for e in range(raw.shape[0])])            # one video per entry
        q = case.queries(6, seed=3)
        ms = ref.query(q, 2, raw.shape[0])
    finally:
        ref.close()
    exp = []
    for f in range(q.shape[0]):
        e = np.nonzero(ms[f] < 1.0)[0]
        exp.append(orc.topk_pairs(ms[f][e], KMAX, e.astype(np.int64)))
    idx = case.index(amd)
    check(idx, q, 2, 20, exp, what="live reference")
    idx.close()


# ------------------------------------------------------------------------------------------ 3 coarseK == 1
def test_single_list_equals_exhaustive_search(amd, orc):
    case = Case(128, 16, 256, 1, seed=21)
    x = case.rows(5000)
    case.x_rot = orc.reorder(case.perm, x)
    case.coarse = case.x_rot[:1].copy() * np.float32(0.5)
    lists, codes = orc.pq_encode(case.x_rot, case.coarse, case.books)
    case.set_entries(lists, codes)
    idx = amd.OpqIndex(case.coarse, case.books, perm=case.perm)
    idx.add_codes(codes[:4000]); idx.add_codes(codes[4000:])
    q = case.queries(40, seed=2)
    for k in (100, 300):
        d0, i0 = idx.search(q, k)
        for d, i in run_both(idx, q, 1, k):
            assert np.array_equal(bits(d), bits(d0)) and np.array_equal(i, i0)
    # and the padding: fewer entries than k
    small = amd.OpqIndex(case.coarse, case.books, perm=case.perm)
    small.add_codes(codes[:150])
    for k in (100, 300):
        d0, i0 = small.search(q, k)
        for d, i in run_both(small, q, 4, k):                            # (nprobe is clamped to 1)
            assert np.array_equal(bits(d), bits(d0)) and np.array_equal(i, i0)
        assert k < 150 or ((i0[:, 150:] == -1).all() and np.isinf(d0[:, 150:]).all())
    idx.close(); small.close()


# ------------------------------------------------------------------------------------------ 4 probe everything
def test_probe_everything(amd, orc):
    base = get_case(orc, "case1")
    case = Case(128, 16, 256, 64, seed=1)
    case.perm, case.books, case.coarse = base.perm, base.books, base.coarse
    lists = base.lists[:3000].copy()
    planted = np.arange(5, 3000, 37)
    lists[planted] = -1                                                   # rows no centroid could claim
    case.set_entries(lists, base.codes[:3000])
    kept = 3000 - planted.size
    idx = case.index(amd)
    q = case.queries(12, seed=4)
    exp = oracle_search(orc, case, q, 64)
    for k in (10, 128, 2048):
        check(idx, q, 64, k, exp, what="probe everything")
    big = amd.OpqIndex(case.coarse, case.books, perm=case.perm)           # fewer kept entries than k
    big.add_codes(base.codes[:900], lists[:900])
    kept = int((lists[:900] >= 0).sum())
    d, i = big.search_ivf(q, 64, 1000)
    assert not np.isin(i, planted).any()
    assert (i[:, :kept] >= 0).all() and np.isfinite(d[:, :kept]).all()
    assert (i[:, kept:] == -1).all() and np.array_equal(bits(d[:, kept:]), bits(np.full((12, 1000 - kept), INF)))
    for f in range(12):
        assert sorted(i[f, :kept].tolist()) == sorted(np.nonzero(lists[:900] >= 0)[0].tolist())
    idx.close(); big.close()


# ------------------------------------------------------------------------------------------ 5 ties across lists
def test_ties_across_lists(amd, orc):
    case = Case(64, 8, 256, 6, seed=31)
    rng = case.rng
    case.coarse = (rng.normal(size=(6, 64)) * 0.05).astype(np.float32)
    a, b, c = 1, 4, 2
    case.coarse[b] = case.coarse[a]                                       # two identical centroids, a < b
    row0 = rng.integers(0, 256, size=8).astype(np.uint8)
    row1 = rng.integers(0, 256, size=8).astype(np.uint8)
    idx = amd.OpqIndex(case.coarse, case.books, perm=case.perm)
    lists, codes = [], []
    for r in range(300):                                                  # identical rows appended alternately to a and b: ids interleave
        blk_l = np.full(1, a if r % 2 == 0 else b, np.int32); blk_c = row0[None, :].copy()
        idx.add_codes(blk_c, blk_l); lists.append(blk_l); codes.append(blk_c)
    filler_c = rng.integers(0, 256, size=(400, 8)).astype(np.uint8)
    filler_l = rng.choice([a, b, c], size=400).astype(np.int32)
    idx.add_codes(filler_c, filler_l); lists.append(filler_l); codes.append(filler_c)
    dup_c = np.repeat(row1[None, :], 300, axis=0); dup_l = np.full(300, c, np.int32)   # 300 copies of one row inside one list
    idx.add_codes(dup_c, dup_l); lists.append(dup_l); codes.append(dup_c)
    case.set_entries(np.concatenate(lists), np.concatenate(codes))
    q_rot = np.stack([case.coarse[a] + np.float32(0.01), case.coarse[c] + np.float32(0.01), (case.coarse[a] + case.coarse[c]) / 2]).astype(np.float32)
    for nprobe in (2, 3, 6):
        exp = oracle_search(orc, case, q_rot, nprobe, rotate=False)
        ks = {1, 2, 7, 100, 128, 129, 299, 300, 301, 1000}
        for f, (ed, ei) in enumerate(exp):                                # a k that cuts every run of equal scores in the middle
            runs = np.nonzero(np.diff(bits(ed)) == 0)[0]
            if runs.size:
                ks.add(int(runs[runs.size // 2]) + 1)
                assert (np.diff(ei)[runs] > 0).all()
        assert any(np.array_equal(bits(ed[k - 1:k]), bits(ed[k:k + 1])) for k in ks for ed, _ in exp if ed.size > k)
        for k in sorted(ks):
            check(idx, q_rot, nprobe, k, exp, rotate=False, what="ties")
    p = probe_lists(q_rot[0], case.coarse, 2)
    assert list(p) == [a, b]                                              # the tied pair is what the first query probes
    idx.close()


# ------------------------------------------------------------------------------------------ 6 skew
def skew_case(rng_seed=41):
    case = Case(128, 16, 256, 16, seed=rng_seed)
    rng = case.rng
    case.coarse = (rng.normal(size=(16, 128)) * 0.05).astype(np.float32)
    case.coarse[9] = case.coarse[3]                                       # list 9 can hold nothing real; kept empty here too
    lists = np.concatenate([np.full(40000, 5), rng.choice([0, 1, 2, 3, 7], size=300), np.full(3, 12)]).astype(np.int32)
    lists = lists[rng.permutation(lists.size)]
    codes = rng.integers(0, 256, size=(lists.size, 16)).astype(np.uint8)
    case.set_entries(lists, codes)
    return case


def skew_queries(case, nq):
    rng = np.random.default_rng(nq)
    target = np.array([5, 5, 9, 4, 12, 5, 15, 3])[np.arange(nq) % 8]       # the long list, empty lists, tiny ones
    return (case.coarse[target] + rng.normal(size=(nq, 128)) * 0.004).astype(np.float32)


@pytest.mark.parametrize("nq", [1, 500])
def test_skewed_lists(amd, orc, nq):
    case = skew_case()
    assert case.longest() == 40000
    idx = case.index(amd)
    q_rot = skew_queries(case, nq)
    for nprobe in (1, 3):
        exp = oracle_search(orc, case, q_rot, nprobe, rotate=False)
        for k in (100, 2048):
            check(idx, q_rot, nprobe, k, exp, rotate=False, what="skew nq=%d" % nq)
            print("skew nq=%d nprobe=%d k=%d: %s" % (nq, nprobe, k, idx.last_ivf_plan()))
    idx.close()


# ------------------------------------------------------------------------------------------ 7 short and empty
def test_short_and_empty(amd, orc):
    case = get_case(orc, "case3")
    q = case.queries(9, seed=6)
    few = Case(32, 4, 200, 40, seed=2)
    few.perm, few.books, few.coarse = case.perm, case.books, case.coarse
    few.set_entries(case.lists[:60], case.codes[:60])
    idx = few.index(amd)
    exp = oracle_search(orc, few, q, 3)
    assert max(e[0].size for e in exp) < 50
    for k in (50, 129, 2048):
        check(idx, q, 3, k, exp, what="short lists")
    idx.close()
    empty = amd.OpqIndex(case.coarse, case.books, perm=case.perm)         # ntotal = 0
    none = amd.OpqIndex(case.coarse, case.books, perm=case.perm)          # every entry in list -1
    none.add_codes(case.codes[:500], np.full(500, -1, np.int32))
    for idx in (empty, none):
        for k in (1, 100, 300):
            for d, i in run_both(idx, q, 3, k):
                assert (i == -1).all() and np.array_equal(bits(d), bits(np.full((9, k), INF)))
        idx.close()


# ------------------------------------------------------------------------------------------ 8 life cycle
def test_life_cycle(amd, orc):
    case = get_case(orc, "case2")
    n = case.lists.size
    q = case.queries(10, seed=8)
    q_rot = orc.reorder(case.perm, q)
    part = Case(64, 8, 256, 200, seed=3)
    part.perm, part.books, part.coarse = case.perm, case.books, case.coarse

    def video_ok(idx, upto):
        part.set_entries(case.lists[:upto], case.codes[:upto])
        want = orc.query_video(q_rot, part.coarse, part.books, 3, part.list_off, part.codes[part.csr_entry], part.csr_entry.astype(np.int32), upto)
        assert np.array_equal(bits(idx.query_video(q, 3, upto)), bits(want))

    idx = amd.OpqIndex(case.coarse, case.books, perm=case.perm)
    idx.add_codes(case.codes[:2501], case.lists[:2501])
    video_ok(idx, 2501)
    assert idx.last_ivf_plan()["entry_bytes"] == 0                        # no id array on a handle that has only run query_video
    check(idx, q, 3, 100, oracle_search(orc, part, q, 3), what="first search")
    assert idx.last_ivf_plan()["entry_bytes"] >= 4 * 2501
    video_ok(idx, 2501)
    idx.add_codes(case.codes[2501:], case.lists[2501:])                   # append at an odd count: ids continue
    part.set_entries(case.lists, case.codes)
    exp = oracle_search(orc, part, q, 3)
    assert max(int(e[1].max()) for e in exp) >= 2501
    check(idx, q, 3, 100, exp, what="after append")
    video_ok(idx, n)
    idx.set_id_base(10 ** 9)
    check(idx, q, 3, 100, oracle_search(orc, part, q, 3, id_base=10 ** 9), what="id base")
    idx.set_id_base(0)
    idx.reset()
    for d, i in run_both(idx, q, 3, 10):
        assert (i == -1).all()
    idx.add_codes(case.codes[1000:1777], case.lists[1000:1777])
    part.set_entries(case.lists[1000:1777], case.codes[1000:1777])
    check(idx, q, 16, 129, oracle_search(orc, part, q, 16), what="after reset")
    want = orc.query_video(q_rot, part.coarse, part.books, 3, part.list_off, part.codes[part.csr_entry], part.csr_entry.astype(np.int32), 777)
    assert np.array_equal(bits(idx.query_video(q, 3, 777)), bits(want))
    off, vid, codes = idx.get_entries()                                   # the list-ordered copy itself is what it was
    assert np.array_equal(off, part.list_off) and np.array_equal(vid, part.csr_entry) and np.array_equal(codes, part.codes[part.csr_entry])
    idx.close()


# ------------------------------------------------------------------------------------------ 9 non-finite
def test_non_finite(amd, orc):
    base = get_case(orc, "case3")                                         # K = 200
    case = Case(32, 4, 200, 40, seed=9)
    case.perm, case.books, case.coarse = base.perm, base.books, base.coarse
    codes = base.codes[:1500].copy()                                      # (fewer than 2048 entries: the +inf ones are part of the longest result)
    planted = np.arange(3, codes.shape[0], 11)
    codes[planted, planted % 4] = 200 + (planted % 56).astype(np.uint8)   # code bytes >= K: +inf scores
    case.set_entries(base.lists[:1500], codes)
    idx = case.index(amd)
    q = case.queries(10, seed=12)
    q[4, 9] = np.inf
    for nprobe, k in ((3, 10), (3, 2048), (40, 100), (40, 2048)):
        exp = oracle_search(orc, case, q, nprobe)
        check(idx, q, nprobe, k, exp, what="non-finite")
    # NaN queries, on codes below K (a planted byte would score +inf where the table holds no NaN): every distance is NaN
    clean = Case(32, 4, 200, 40, seed=9)
    clean.perm, clean.books, clean.coarse = base.perm, base.books, base.coarse
    clean.set_entries(base.lists[:1500], base.codes[:1500])
    cidx = clean.index(amd)
    qn = q.copy()
    qn[2, 5] = np.nan
    qn[7, :] = np.nan
    for nprobe, k in ((3, 10), (3, 2048), (40, 100), (40, 2048)):
        exp = oracle_search(orc, clean, qn, nprobe)
        assert np.isnan(exp[2][0]).all() and np.isnan(exp[7][0]).all()
        check(cidx, qn, nprobe, k, exp, nan_rows=(2, 7), what="NaN queries")
    cidx.close()
    exp = oracle_search(orc, case, q, 40)
    d, i = idx.search_ivf(q, 40, 2048)
    ed, ei = exp[0]
    inf_at = np.nonzero(np.isinf(ed))[0]
    assert inf_at.size > 0 and inf_at[0] > 0 and np.isfinite(ed[:inf_at[0]]).all()   # +inf scores rank after every finite one ...
    assert (np.diff(ei[inf_at]) > 0).all() and set(ei[inf_at].tolist()) <= set(planted.tolist())   # ... by id ...
    assert (i[0, :ed.size] >= 0).all() and (i[0, ed.size:] == -1).all()   # ... ahead of the padding
    assert np.isinf(exp[4][0]).all()                                      # the inf query: every entry scores +inf, ids ascending
    idx.close()


# ------------------------------------------------------------------------------------------ 10 grid shapes
def test_grid_shapes(amd, orc):
    case = get_case(orc, "case1")
    idx = case.index(amd)
    seen = set()
    qall = case.queries(5000, seed=13)
    expall = oracle_search(orc, case, qall, 3)
    for nq in (1, 7, 64, 1000, 5000):
        for k in (10, 300):
            check(idx, qall[:nq], 3, k, expall[:nq], what="grid nq=%d" % nq)
            p = idx.last_ivf_plan()
            print("nq=%d nprobe=3 k=%d: rule %d, G=%d groups=%d pieces=%d x %d rows, %d partial lists (%d bytes)" % (
                nq, k, p["rule"], p["G"], p["groups"], p["pieces"], p["rows_per_piece"], p["parts"], p["part_bytes"]))
            seen.add(p["rule"])
    assert idx.last_ivf_plan()["parts"] == 1
    idx.close()
    case2 = get_case(orc, "case2")                                        # 200 lists: nq = 2 at nprobe = 128
    idx = case2.index(amd)
    q = case2.queries(2, seed=14)
    exp = oracle_search(orc, case2, q, 128)
    for k in (10, 300, 2048):
        check(idx, q, 128, k, exp, what="grid nprobe=128")
        p = idx.last_ivf_plan()
        print("nq=2 nprobe=128 k=%d: rule %d, G=%d groups=%d pieces=%d, %d partial lists" % (k, p["rule"], p["G"], p["groups"], p["pieces"], p["parts"]))
        seen.add(p["rule"])
    amd.set_tuning("ivf_part_cap_mb", 1)                                  # the partial lists have to fit: a coarser grid
    try:
        check(idx, q, 128, 2048, exp, what="grid rule 4")
        p = idx.last_ivf_plan()
        print("nq=2 nprobe=128 k=2048 under a 1 MB cap: rule %d, groups=%d, %d bytes" % (p["rule"], p["groups"], p["part_bytes"]))
        assert p["part_bytes"] <= 1 << 20
        seen.add(p["rule"])
        amd.set_tuning("ivf_part_cap_mb", 0)
        check(idx, q, 128, 2048, exp, what="grid no partial lists")
        assert idx.last_ivf_plan()["parts"] == 1
    finally:
        amd.set_tuning("ivf_part_cap_mb", 256)
    idx.close()
    assert seen == {1, 2, 3, 4}, seen
    with pytest.raises(amd.CvtmiError):                                   # nprobe above 128 after the clamp
        case2.index(amd).search_ivf(q, 129, 10)


@pytest.mark.parametrize("name", ["case2", "case3", "odd"])
def test_one_workgroup_per_query_at_other_widths(amd, orc, name):
    """600 queries make one workgroup per query walk all its lists (rule 1): M = 8, 4 and 2, K < 256, tables rebuilt list after list."""
    case = get_case(orc, name)
    idx = case.index(amd)
    q = case.queries(600, seed=17)
    nprobe = min(3, case.coarseK)
    exp = oracle_search(orc, case, q, nprobe)
    for k in (10, 129):
        check(idx, q, nprobe, k, exp, what=name)
        assert idx.last_ivf_plan()["G"] == nprobe and idx.last_ivf_plan()["parts"] == 1
    idx.close()


# ------------------------------------------------------------------------------------------ 11 concurrency
def test_concurrent_searches(amd, orc):
    case = get_case(orc, "case1")
    idx = case.index(amd)
    q = case.queries(300, seed=15)
    jobs = [(1, 10), (3, 100), (16, 300), (64, 2048)]
    serial = [idx.search_ivf(q, nprobe, k) for nprobe, k in jobs]
    got = [None] * len(jobs)
    errs = []

    def work(j):
        try:
            for _ in range(4):
                got[j] = idx.search_ivf(q, *jobs[j])
        except Exception as e:   # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=work, args=(j,)) for j in range(len(jobs))]
    for t in ts: t.start()
    for t in ts: t.join()
    assert not errs, errs
    for (d0, i0), (d, i) in zip(serial, got):
        assert np.array_equal(bits(d0), bits(d)) and np.array_equal(i0, i)
    exp = oracle_search(orc, case, q[:20], 16)
    ed, ei = padded(exp, 300)
    assert np.array_equal(bits(got[2][0][:20]), bits(ed)) and np.array_equal(got[2][1][:20], ei)
    idx.close()


# ------------------------------------------------------------------------------------------ 12 full size
def test_full_size(amd, orc):
    import torch
    from cvt_amd import synth
    D, M, K, L, n, nq, nprobe, k = 128, 16, 256, 8192, 1000000, 1000, 16, 100
    x = synth.sift_like(n, D, device="cuda")
    q = synth.sift_like(nq, D, seed=0xBEEF, device="cuda")
    perm = synth.random_permutation(D)
    sel = torch.randperm(n, generator=torch.Generator().manual_seed(5))[:L].cuda()
    probe = amd.OpqIndex(np.zeros((1, D), np.float32), np.zeros((M, K, D // M), np.float32), perm=perm)
    xr = probe.rotate(x)
    coarse = xr[sel].cpu().numpy()
    res = (xr[:65536] - xr[sel[torch.randint(0, L, (65536,), generator=torch.Generator().manual_seed(6)).cuda()]])
    books = synth.train_books(res, M, K, iters=2)
    probe.close()
    idx = amd.OpqIndex(coarse, books, perm=perm)
    lists, codes = idx.encode(xr)
    idx.add_codes(codes, lists)
    d, i = idx.search_ivf(q, nprobe, k)
    torch.cuda.synchronize()
    print("full size: %s" % idx.last_ivf_plan())
    d, i = d.cpu().numpy(), i.cpu().numpy()
    case = Case(D, M, K, L, seed=0)
    case.perm, case.books, case.coarse = np.asarray(perm, np.int32), np.asarray(books, np.float32), coarse
    case.set_entries(lists.cpu().numpy(), codes.cpu().numpy())
    print("full size: longest list %d, empty lists %d" % (case.longest(), int((np.diff(case.list_off) == 0).sum())))
    pick = np.linspace(0, nq - 1, 20).astype(int)
    qn = q.cpu().numpy()
    exp = oracle_search(orc, case, qn[pick], nprobe)
    ed, ei = padded(exp, k)
    assert np.array_equal(bits(d[pick]), bits(ed)) and np.array_equal(i[pick], ei)
    assert (i >= 0).all() and (i < n).all()
    assert all(len(set(row.tolist())) == k for row in i)
    assert (np.diff(d, axis=1) >= 0).all()
    idx.close()


# ------------------------------------------------------------------------------------------ 13 host layers
def test_host_layers(tmp_path, amd, orc, golden):
    """opq_search --nprobe 3 (IVFOPQ::SearchTopKProbe underneath) on the golden IVF model and data returns the ABI's lists."""
    exe = os.path.join(BIN, "opq_search")
    assert os.path.exists(exe), "host CLIs not built: __graft_entry__.build()"
    g = golden.opq["opq_ivf"]
    model = str(tmp_path / "model.bin")
    ob.write_opq_model(model, g["coarse"], g["books"], g["perm"])
    np.ascontiguousarray(g["db"], np.float32).tofile(str(tmp_path / "db.bin"))
    np.ascontiguousarray(g["queries"], np.float32).tofile(str(tmp_path / "q.bin"))
    k = 20
    r = subprocess.run([exe, model, "db.bin", "q.bin", "res.txt", "--k", str(k), "--nprobe", "3"], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = (tmp_path / "res.txt").read_text().splitlines()
    nq = g["queries"].shape[0]
    assert len(lines) == nq
    idx = amd.OpqIndex(g["coarse"], g["books"], perm=g["perm"])
    lists, codes = idx.rotate_encode(g["db"])
    idx.add_codes(codes, lists)
    d, i = idx.search_ivf(g["queries"], 3, k)
    case = Case(32, 4, 256, 16, seed=0)                                   # and the oracle, on the golden codes' own lists
    case.perm, case.books, case.coarse = g["perm"], g["books"], g["coarse"]
    case.set_entries(lists, codes)
    assert np.array_equal(case.list_off, g["list_off"])
    ed, ei = padded(oracle_search(orc, case, g["queries"], 3), k)
    assert np.array_equal(bits(d), bits(ed)) and np.array_equal(i, ei)
    for f, line in enumerate(lines):
        head, rest = line.split(" topK: ")
        ids_s, d_s = rest.split("dists: ")
        assert int(head) == f
        assert [int(t) for t in ids_s.split()] == i[f].tolist()
        assert np.array_equal(bits(np.array([float(t) for t in d_s.split()], np.float32)), bits(d[f]))   # %.9g round-trips fp32
    # without --nprobe the CLI is what it was: a coarseK > 1 model is refused
    r = subprocess.run([exe, model, "db.bin", "q.bin", "res2.txt", "--k", str(k)], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "coarseK == 1" in r.stderr
    idx.close()
