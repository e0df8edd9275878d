"""GPU: cvtmi_flat_rerank (csrc/flat_rerank.hip), cvtmi_opq_search_refine and the layers above them.

Every comparison is exact: uint32 views of the distances, equality of the labels.  Expectations never come from the code under test:
  fp32   orc.dist(metric, flavour, q, row) per pair, flavour 4 for IP and 8 for L2F (as test_gpu_flat_range.py);
  uint8  numpy int64 ((q - x) ** 2)[: D // 4 * 4].sum();
then Python set logic over a query's candidates (arbitrary-precision integers: no overflow at the int64 extremes) and np.lexsort by
(distance, row).  Rows hold exact duplicates, so ties by row occur, and q[0] = rows[0].

Shapes: n around the 64-row block of the fp32 layout and past several tiles of the kernel (a 128-d tile holds 30 rows); fp32 at D = 4,
32, 128 (blocked rows, or their row-major copy) and 37 (row-major, scalar loop), uint8 at D = 32, 48 (16-byte units) and 5 (single
bytes, tail dropped); R from 1 over the 64-lane wave and the 256-thread workgroup to 4096, the LDS sort's largest size."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IP, L2F, L2U8 = 0, 1, 2
LAYOUTS = [(IP, 4), (IP, 32), (IP, 128), (IP, 37), (L2F, 4), (L2F, 32), (L2F, 128), (L2F, 37), (L2U8, 32), (L2U8, 48), (L2U8, 5)]
LABEL_MODES = ["implicit", "implicit_base", "explicit", "explicit_x3"]
NS = [1, 63, 64, 65, 257, 1025]
NQS = [1, 5, 33]
RS = [1, 2, 63, 64, 65, 1000, 4096]
BASES = [0, 10 ** 10, -7]
BASE = 10 ** 10
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
PAD = 0x7f800000
CVTMI_EINVAL = -1
LANES = {(IP, 4): 4, (IP, 32): 4, (IP, 128): 4, (IP, 37): 1, (L2F, 4): 4, (L2F, 32): 8, (L2F, 128): 8, (L2F, 37): 1,
         (L2U8, 32): 0, (L2U8, 48): 0, (L2U8, 5): 0}


@pytest.fixture(scope="module")
def amd():
    import torch
    torch.cuda.is_available()
    import cvt_amd
    return cvt_amd


def blocked(metric, D):
    return metric != L2U8 and D % 4 == 0


def make_rows(metric, n, D, seed):
    """rows with exact duplicates in them (test_gpu_flat_range.py's): ties by row at every rank"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(n, D), dtype=np.uint8) if metric == L2U8 else rng.normal(size=(n, D)).astype(np.float32)
    for j in range(3, n, 7):
        x[j] = x[j % 3]
    return x


def make_queries(metric, D, seed, nq, rows=None):
    rng = np.random.default_rng(seed + 77)
    q = rng.integers(0, 256, size=(nq, D), dtype=np.uint8) if metric == L2U8 else rng.normal(size=(nq, D)).astype(np.float32)
    if rows is not None and len(rows):
        q[0] = rows[0]
    return q


def make_labels(mode, n, seed):
    """(labels to add with or None, id_base, the labels the searches report)"""
    if mode == "implicit":
        return None, 0, np.arange(n, dtype=np.int64)
    if mode == "implicit_base":
        return None, BASE, BASE + np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(seed + 5)
    lab = rng.choice(np.arange(-4 * n - 8, 4 * n + 8), size=n, replace=False).astype(np.int64)
    lab[::5] += 2 ** 33
    if n >= 3:
        lab[n // 2] = I64_MIN
        lab[n - 1] = I64_MAX
    if mode == "explicit_x3" and n >= 9:
        lab[n // 3] = lab[2 * n // 3] = lab[1]
    return lab, 0, lab.copy()


def build(amd, metric, D, rows, labels=None, base=0, copy=0):
    ix = amd.FlatIndex(metric, D)
    if base:
        ix.set_id_base(base)
    if copy:
        ix.set_param("rerank_rows_copy", copy)
    if len(rows):
        ix.add(rows, labels)
    return ix


_E = {}


def dist_matrix(orc, metric, x, q, tag=None):
    """E[query][row]: the distance cvtmi_flat_search reports for the pair, from the CPU oracle / numpy (kept per tag: computed once)"""
    if tag is not None and tag in _E:
        return _E[tag]
    if metric == L2U8:
        d4 = x.shape[1] // 4 * 4
        xi, qi = x[:, :d4].astype(np.int64), q[:, :d4].astype(np.int64)
        E = np.stack([((xi - one) ** 2).sum(axis=1) for one in qi]).astype(np.int32).reshape(len(q), len(x))
    else:
        flavour = 4 if metric == IP else 8
        E = np.array([orc.dist(metric, flavour, one, r) for one in q for r in x], dtype=np.float32).reshape(len(q), len(x))
    if tag is not None:
        _E[tag] = E
    return E


def make_cands(n, nq, R, base, seed):
    """[nq][R] int64: random valid rows with repeats; -1, n, n + 5 shifted by the base, the unshifted -1 of a padded search and the two
    int64 extremes sprinkled over them.  Query 1 names no valid row at all, query 2 only three distinct ones."""
    rng = np.random.default_rng(seed)
    special = [base - 1, base + n, base + n + 5, -1, I64_MIN, I64_MAX]
    special = [s for s in special if I64_MIN <= s <= I64_MAX]
    cand = np.empty((nq, R), dtype=object)
    for f in range(nq):
        row = [base + int(r) for r in rng.integers(0, max(n, 1), size=R)] if n else [base + 3] * R
        if f == 1:
            row = [special[j % len(special)] for j in range(R)]
        elif f == 2 and n:
            few = [base + int(r) for r in rng.integers(0, n, size=3)]
            row = [few[j % 3] for j in range(R)]
        for j in rng.choice(R, size=min(R, max(1, R // 4)) if R > 1 else int(rng.integers(0, 2)), replace=False):
            row[j] = special[int(rng.integers(0, len(special)))]
        if f == 1:
            row = [s if not (base <= s < base + n) else base + n for s in row]   # (base = -7: the unshifted -1 names row 6)
        cand[f] = row
    return np.array(cand.tolist(), dtype=np.int64).reshape(nq, R)


def expect(metric, E, reported, cand, base, k):
    """(distance bits [nq][k] uint32, labels [nq][k]): the k smallest (distance, row) over the distinct valid rows of every query"""
    nq, n = E.shape
    bits = np.full((nq, k), PAD, np.uint32)
    labels = np.full((nq, k), -1, np.int64)
    for f in range(nq):
        rows = sorted({int(c) - base for c in cand[f].tolist() if base <= int(c) < base + n})
        if not rows:
            continue
        rows = np.array(rows, dtype=np.int64)
        d = E[f, rows]
        assert not np.isnan(d.astype(np.float64)).any()
        order = np.lexsort((rows, d))[:k]           # (numpy compares -0.0 == +0.0, as the kernel's keys do)
        bits[f, :len(order)] = np.ascontiguousarray(d[order]).view(np.uint32)
        labels[f, :len(order)] = reported[rows[order]]
    return bits, labels


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run(ix, q, cand, k, base, dev=False):
    if not dev:
        return ix.rerank(q, cand, k, cand_base=base)
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d, i = ix.rerank(torch.from_numpy(q).cuda(), torch.from_numpy(cand).cuda(), k, cand_base=base)
    s.synchronize()            # the one wait
    return d.cpu().numpy(), i.cpu().numpy()


def check(ix, metric, q, cand, k, base, E, reported, what, dev=False, source=None):
    eb, el = expect(metric, E, reported, cand, base, k)
    d, i = run(ix, q, cand, k, base, dev)
    assert d.dtype == (np.int32 if metric == L2U8 else np.float32) and d.shape == eb.shape
    assert np.array_equal(u32(d), eb), what
    assert np.array_equal(i, el), what
    if source is not None:
        assert ix.last_rerank()[0] == source, (what, ix.last_rerank())
    return d, i


def pick_k(turn, R):
    return min([1, 10, R, R + 3, 2048][turn % 5], 2048)     # (R = 4096: k stops at CVTMI_K_MAX)


# ---- 1. every layout at the row counts around block and tile; R, k, batch size, base, label mode and entry rotate through the grid ----
@pytest.mark.parametrize("metric,D", LAYOUTS)
def test_shapes_candidates_and_sources(amd, orc, metric, D):
    turn = LAYOUTS.index((metric, D))
    for n in NS:
        mode = LABEL_MODES[turn % 4]
        nq = NQS[turn % 3]
        R = RS[(turn * 3 + 1) % 7]
        k = pick_k(turn // 2, R)
        base = BASES[(turn // 3) % 3]
        dev = turn % 4 == 3
        turn += 1
        rows = make_rows(metric, n, D, seed=n + D)
        q = make_queries(metric, D, n, nq, rows=rows)
        labels, id_base, reported = make_labels(mode, n, seed=n)
        E = dist_matrix(orc, metric, rows, q)
        cand = make_cands(n, nq, R, base, seed=turn)
        what = (metric, D, n, nq, R, k, base, mode, dev)
        ix = build(amd, metric, D, rows, labels, id_base)
        d0, i0 = check(ix, metric, q, cand, k, base, E, reported, what, dev=dev, source=1 if blocked(metric, D) else 0)
        info = ix.last_rerank()
        assert info[1] == LANES[(metric, D)] and info[2] == nq and 0 < info[3] <= 96 * 1024, (what, info)
        if nq > 1:
            assert (i0[1] == -1).all() and (u32(d0[1]) == PAD).all(), what                       # no valid candidate: all padding
        if nq > 2 and k > 4:
            assert (u32(d0[2, 4:]) == PAD).all() and u32(d0[2, 0]) != PAD, what      # three distinct rows (four where the unshifted -1 names one), then padding
        ix.close()
        if blocked(metric, D):
            ix = build(amd, metric, D, rows, labels, id_base, copy=1)
            d1, i1 = check(ix, metric, q, cand, k, base, E, reported, what, dev=not dev, source=2)
            assert np.array_equal(u32(d0), u32(d1)) and np.array_equal(i0, i1), what
            ix.close()


# ---- 2. the remaining corners of (R, k) on one table per row source ----
@pytest.mark.parametrize("metric,D,copy", [(L2F, 128, 0), (L2F, 128, 1), (IP, 37, 0), (L2U8, 32, 0), (L2U8, 5, 0)])
def test_every_r_and_k_on_one_table(amd, orc, metric, D, copy):
    n, nq = 257, 5
    rows = make_rows(metric, n, D, seed=D)
    q = make_queries(metric, D, 5, nq, rows=rows)
    E = dist_matrix(orc, metric, rows, q, tag=("one", metric, D))
    labels, id_base, reported = make_labels("explicit_x3", n, seed=2)
    ix = build(amd, metric, D, rows, labels, id_base, copy=copy)
    for turn, R in enumerate(RS):
        cand = make_cands(n, nq, R, BASES[turn % 3], seed=R)
        for k in sorted({1, 10, R, R + 3, 2048}):
            if k <= 2048:
                check(ix, metric, q, cand, k, BASES[turn % 3], E, reported, (metric, D, R, k), dev=(turn + k) % 3 == 0,
                      source=(2 if copy else 1) if blocked(metric, D) else 0)
    ix.close()


@pytest.mark.parametrize("metric,D", [(L2F, 4096), (IP, 4095), (L2U8, 4096)])
def test_widest_rows_largest_lists(amd, orc, metric, D):
    """the most LDS a workgroup asks for: 4096 pairs, a one-row tile, a 16 KB query"""
    n, nq, R, k = 65, 2, 4096, 2048
    rows = make_rows(metric, n, D, seed=D)
    q = make_queries(metric, D, 3, nq, rows=rows)
    E = dist_matrix(orc, metric, rows, q)
    reported = np.arange(n, dtype=np.int64)
    for copy in ((0, 1) if blocked(metric, D) else (0,)):
        ix = build(amd, metric, D, rows, copy=copy)
        check(ix, metric, q, make_cands(n, nq, R, -7, seed=D), k, -7, E, reported, (metric, D, copy),
              source=(2 if copy else 1) if blocked(metric, D) else 0)
        assert ix.last_rerank()[3] > 48 * 1024
        ix.close()


# ---- 3. order and multiplicity of a list do not matter; the result is cvtmi_flat_search's on the distinct valid rows ----
@pytest.mark.parametrize("metric,D", [(IP, 32), (L2F, 37), (L2U8, 48)])
def test_permutation_duplication_and_flat_search_equivalence(amd, orc, metric, D):
    n, nq, R, k = 257, 5, 65, 10
    rows = make_rows(metric, n, D, seed=D + 3)
    q = make_queries(metric, D, 9, nq, rows=rows)
    labels, id_base, reported = make_labels("explicit", n, seed=4)
    ix = build(amd, metric, D, rows, labels, id_base)
    rng = np.random.default_rng(D)
    for base in BASES:
        cand = make_cands(n, nq, R, base, seed=base % 97)
        d0, i0 = ix.rerank(q, cand, k, cand_base=base)
        shuffled = np.stack([rng.permutation(c) for c in cand])
        doubled = np.concatenate([shuffled, cand[:, ::-1], cand[:, :7]], axis=1)
        for other in (shuffled, doubled):
            d1, i1 = ix.rerank(q, other, k, cand_base=base)
            assert np.array_equal(u32(d0), u32(d1)) and np.array_equal(i0, i1), (metric, D, base, other.shape)
        for f in (0, 3):   # a fresh handle that holds only f's distinct valid rows, in ascending row order, with the labels they report
            sub = np.array(sorted({int(c) - base for c in cand[f].tolist() if base <= int(c) < base + n}), dtype=np.int64)
            fresh = build(amd, metric, D, rows[sub], reported[sub])
            sd, si = fresh.search(q[f:f + 1], k)
            assert np.array_equal(u32(sd[0]), u32(d0[f])) and np.array_equal(si[0], i0[f]), (metric, D, base, f)
            fresh.close()
    ix.close()


# ---- 4. the row-major copy: stale after an add, extended on request, gone after a removal ----
@pytest.mark.parametrize("metric,D", [(L2F, 32), (IP, 128)])
def test_rows_copy_follows_the_index(amd, orc, metric, D):
    n0, more, nq, R, k = 257, 100, 5, 64, 10
    n = n0 + more
    rows = make_rows(metric, n, D, seed=D + 11)
    q = make_queries(metric, D, 2, nq, rows=rows)
    E = dist_matrix(orc, metric, rows, q)
    reported = BASE + np.arange(n, dtype=np.int64)
    ix = build(amd, metric, D, rows[:n0], None, BASE, copy=1)
    cand = make_cands(n0, nq, R, 0, seed=1)
    check(ix, metric, q, cand, k, 0, E[:, :n0], reported[:n0], "copy built", source=2)
    ix.set_param("rerank_rows_copy", 0)
    ix.add(rows[n0:])
    cand = make_cands(n, nq, R, 0, seed=2)
    cand[:, :8] = np.arange(n - 8, n)                        # rows beyond the old count, for every query but the all-invalid one
    cand[1, :8] = -1
    check(ix, metric, q, cand, k, 0, E, reported, "stale copy is not read", source=1)
    ix.set_param("rerank_rows_copy", 1)
    check(ix, metric, q, cand, k, 0, E, reported, "copy extended", source=2)
    rng = np.random.default_rng(D)
    keep = rng.random(n) >= 0.4
    assert ix.remove_labels(reported[~keep]) == int((~keep).sum())
    nk = int(keep.sum())
    fresh = build(amd, metric, D, rows[keep], reported[keep])
    cand = make_cands(nk, nq, R, 0, seed=3)
    for param, source in ((0, 1), (1, 2)):
        ix.set_param("rerank_rows_copy", param)
        d, i = check(ix, metric, q, cand, k, 0, E[:, keep], reported[keep], ("after remove_labels", param), source=source)
        fd, fi = fresh.rerank(q, cand, k)
        assert np.array_equal(u32(d), u32(fd)) and np.array_equal(i, fi)
    ix.close(); fresh.close()


# ---- 5. a NaN query: min(k, distinct valid rows) distinct rows, all with NaN distances ----
@pytest.mark.parametrize("metric,D,copy", [(IP, 32, 0), (L2F, 128, 1), (L2F, 37, 0)])
def test_nan_query(amd, orc, metric, D, copy):
    n, nq, R = 257, 5, 65
    rows = make_rows(metric, n, D, seed=D)
    q = make_queries(metric, D, 1, nq, rows=rows)
    q[3, :] = np.nan
    ix = build(amd, metric, D, rows, None, BASE, copy=copy)
    cand = make_cands(n, nq, R, 0, seed=8)
    valid = sorted({int(c) for c in cand[3].tolist() if 0 <= int(c) < n})
    assert len(valid) > 12
    for k in (10, R + 3):
        d, i = ix.rerank(q, cand, k)
        m = min(k, len(valid))
        assert np.isnan(d[3, :m]).all() and len(set(i[3, :m].tolist())) == m and set(i[3, :m].tolist()) <= {BASE + r for r in valid}
        assert (i[3, m:] == -1).all() and (u32(d[3, m:]) == PAD).all()
        if m == len(valid):
            assert set(i[3, :m].tolist()) == {BASE + r for r in valid}
        finite = [0, 1, 2, 4]                                                   # the other queries are untouched by their neighbour
        E = dist_matrix(orc, metric, rows, q[finite], tag=("nan", metric, D))
        eb, el = expect(metric, E, BASE + np.arange(n, dtype=np.int64), cand[finite], 0, k)
        assert np.array_equal(u32(d[finite]), eb) and np.array_equal(i[finite], el)
    ix.close()


# ---- 6. limits: an empty index pads everything, nq == 0 does nothing, the ranges of k and R ----
def test_empty_index_and_limits(amd):
    import torch
    from cvt_amd.capi import CvtmiError, _ptr, _stream
    lib = amd.lib()
    for metric, D in ((L2F, 32), (L2U8, 5)):
        empty = amd.FlatIndex(metric, D)
        q = make_queries(metric, D, 0, 3)
        cand = np.array([[0, -1, 5, I64_MAX], [I64_MIN, 0, 0, 1], [3, 2, 1, 0]], dtype=np.int64)
        for dev in (False, True):
            d, i = run(empty, q, cand, 6, 0, dev)
            assert (i == -1).all() and (u32(d) == PAD).all()
        empty.close()
    rows = make_rows(L2F, 65, 32, seed=1)
    ix = build(amd, L2F, 32, rows)
    q = make_queries(L2F, 32, 0, 2, rows=rows)
    cand = np.zeros((2, 4), np.int64)
    d = np.full((2, 3), 7.0, np.float32); i = np.full((2, 3), -7, np.int64)
    assert lib.cvtmi_flat_rerank(ix.h, _ptr(q), C.c_int64(0), _ptr(cand), C.c_int(4), C.c_int64(0), C.c_int(3), _ptr(d), _ptr(i)) == 0
    assert lib.cvtmi_flat_rerank_dev(ix.h, None, C.c_int64(0), None, C.c_int(4), C.c_int64(0), C.c_int(3), None, None, _stream()) == 0
    torch.cuda.synchronize()
    assert (d == 7.0).all() and (i == -7).all()
    for R, k in ((0, 3), (4097, 3), (4, 0), (4, 2049)):
        assert lib.cvtmi_flat_rerank(ix.h, _ptr(q), C.c_int64(2), _ptr(cand), C.c_int(R), C.c_int64(0), C.c_int(k), _ptr(d), _ptr(i)) == CVTMI_EINVAL
    assert (d == 7.0).all() and (i == -7).all()
    with pytest.raises(CvtmiError):
        ix.set_param("rerank_rows_copy", 2)
    ix.close()


# ---- 7. two threads rerank different batches on one handle while a third searches ----
@pytest.mark.parametrize("metric,D,copy", [(L2F, 32, 1), (L2U8, 32, 0)])
def test_threads_on_one_handle(amd, orc, metric, D, copy):
    n, nq, R, k = 1025, 5, 1000, 10
    rows = make_rows(metric, n, D, seed=D + 2)
    reported = np.arange(n, dtype=np.int64)
    ix = build(amd, metric, D, rows, copy=copy)
    batches = []
    for t in range(3):
        q = make_queries(metric, D, 8 + t, nq, rows=rows)
        E = dist_matrix(orc, metric, rows, q)
        cand = make_cands(n, nq, R, BASES[t], seed=t)
        batches.append((q, cand, BASES[t], expect(metric, E, reported, cand, BASES[t], k), E))
    got, errors = [None] * 3, []

    def work(t):
        try:
            q, cand, base = batches[t][:3]
            got[t] = [ix.search(q, k) if t == 2 else ix.rerank(q, cand, k, cand_base=base) for _ in range(6)]
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for t in range(2):
        eb, el = batches[t][3]
        for d, i in got[t]:
            assert np.array_equal(u32(d), eb) and np.array_equal(i, el)
    E = batches[2][4]
    order = np.stack([np.lexsort((np.arange(n), E[f]))[:k] for f in range(nq)])
    for d, i in got[2]:
        assert np.array_equal(i, order) and np.array_equal(u32(d), u32(np.take_along_axis(E, order, axis=1)))
    ix.close()


# ---- 8. refine: ADC candidates from the OPQ index, exact finish against the flat index ----
class Refine:
    D, M, K, n, nq = 32, 4, 256, 2000, 9

    def __init__(self, orc):
        rng = np.random.default_rng(31)
        D, M, K, n = self.D, self.M, self.K, self.n
        centres = rng.normal(size=(12, D)) * 0.03
        self.x = (centres[rng.integers(0, 12, size=n)] * 0.7 + rng.normal(size=(n, D)) * 0.02).astype(np.float32)
        self.x[5::11] = self.x[2]                                   # exact duplicates: ties in both stages
        self.q = (centres[rng.integers(0, 12, size=self.nq)] * 0.7 + rng.normal(size=(self.nq, D)) * 0.02).astype(np.float32)
        self.q[0] = self.x[2]
        self.perm = rng.permutation(D).astype(np.int32)
        self.books = (rng.normal(size=(M, K, D // M)) * 0.03).astype(np.float32)
        self.x_rot = orc.reorder(self.perm, self.x)
        self.q_rot = orc.reorder(self.perm, self.q)
        self.coarse1 = np.zeros((1, D), np.float32)
        self.coarse16 = self.x_rot[rng.choice(n, size=16, replace=False)].copy()
        _, self.codes1 = orc.pq_encode(self.x_rot, self.coarse1, self.books)
        self.lists16, self.codes16 = orc.pq_encode(self.x_rot, self.coarse16, self.books)
        self.E = {m: np.array([orc.dist(m, 4 if m == IP else 8, one, r) for one in self.q for r in self.x], dtype=np.float32).reshape(self.nq, n)
                  for m in (IP, L2F)}

    def opq(self, amd, coarseK, id_base=0):
        if coarseK == 1:
            ix = amd.OpqIndex(self.coarse1, self.books, perm=self.perm)
            ix.add_codes(self.codes1)
        else:
            ix = amd.OpqIndex(self.coarse16, self.books, perm=self.perm)
            ix.add_codes(self.codes16, self.lists16)
        if id_base:
            ix.set_id_base(id_base)
        return ix


@pytest.fixture(scope="module")
def refine(orc):
    return Refine(orc)


KR = [(1, 10), (10, 64), (10, 2048)]


@pytest.mark.parametrize("metric", [IP, L2F])
def test_refine_exhaustive_scan(amd, orc, refine, metric):
    """nprobe = 0: the composition of search and rerank, and the oracle chain adc_search -> dist -> lexsort"""
    c = refine
    labels, _, reported = make_labels("explicit", c.n, seed=6)
    flat = build(amd, metric, c.D, c.x, labels)
    for id_base in (0, BASE):
        opq = c.opq(amd, 1, id_base)
        for k, R in KR:
            cd, ci = opq.search(c.q, R)
            d0, i0 = flat.rerank(c.q, ci, k, cand_base=id_base)
            _, oi = orc.adc_search(c.q_rot, c.books, c.codes1, min(R, c.n))
            if R > c.n:
                oi = np.concatenate([oi, np.full((c.nq, R - c.n), -1, np.int64)], axis=1)
            eb, el = expect(metric, c.E[metric], reported, oi, 0, k)
            assert np.array_equal(u32(d0), eb) and np.array_equal(i0, el), (metric, id_base, k, R)
            for dev in (False, True):
                if dev:
                    import torch
                    s = torch.cuda.Stream()
                    with torch.cuda.stream(s):
                        d, i = opq.search_refine(flat, torch.from_numpy(c.q).cuda(), k, R)
                    s.synchronize()
                    d, i = d.cpu().numpy(), i.cpu().numpy()
                else:
                    d, i = opq.search_refine(flat, c.q, k, R)
                assert np.array_equal(u32(d), u32(d0)) and np.array_equal(i, i0), (metric, id_base, k, R, dev)
        opq.close()
    flat.close()


@pytest.mark.parametrize("nprobe", [1, 3, 16])
def test_refine_ivf(amd, refine, nprobe):
    c = refine
    flat = build(amd, L2F, c.D, c.x, None, 5 * BASE, copy=1 if nprobe == 3 else 0)
    reported = 5 * BASE + np.arange(c.n, dtype=np.int64)
    for id_base in (0, BASE):
        opq = c.opq(amd, 16, id_base)
        for k, R in KR:
            cd, ci = opq.search_ivf(c.q, nprobe, R)
            d0, i0 = flat.rerank(c.q, ci, k, cand_base=id_base)
            eb, el = expect(L2F, c.E[L2F], reported, ci, id_base, k)      # (the candidates are the IVF search's; the finish is the oracle's)
            assert np.array_equal(u32(d0), eb) and np.array_equal(i0, el), (nprobe, id_base, k, R)
            d, i = opq.search_refine(flat, c.q, k, R, nprobe=nprobe)
            assert np.array_equal(u32(d), u32(d0)) and np.array_equal(i, i0), (nprobe, id_base, k, R)
            d, i = opq.search_refine(flat, c.q, k, R, nprobe=nprobe, rotate=False)      # rotate steers the scan only
            cd, ci = opq.search_ivf(c.q, nprobe, R, rotate=False)
            d1, i1 = flat.rerank(c.q, ci, k, cand_base=id_base)
            assert np.array_equal(u32(d), u32(d1)) and np.array_equal(i, i1), (nprobe, id_base, k, R, "unrotated")
        opq.close()
    flat.close()


def test_refine_mismatches(amd, refine):
    from cvt_amd.capi import CvtmiError
    c = refine
    opq1, opq16 = c.opq(amd, 1), c.opq(amd, 16)
    good = build(amd, L2F, c.D, c.x)
    assert good.ntotal == c.n
    wrong_d = build(amd, L2F, c.D + 4, np.zeros((c.n, c.D + 4), np.float32))
    wrong_n = build(amd, L2F, c.D, c.x[:-1])
    wrong_m = build(amd, L2U8, c.D, np.zeros((c.n, c.D), np.uint8))
    for opq, nprobe in ((opq1, 0), (opq16, 3)):
        for flat in (wrong_d, wrong_n, wrong_m):
            with pytest.raises(CvtmiError) as err:
                opq.search_refine(flat, c.q, 3, 10, nprobe=nprobe)
            assert err.value.code == CVTMI_EINVAL
        for k, R in ((0, 10), (11, 10), (3, 2049)):
            with pytest.raises(CvtmiError) as err:
                opq.search_refine(good, c.q, k, R, nprobe=nprobe)
            assert err.value.code == CVTMI_EINVAL
    with pytest.raises(CvtmiError) as err:
        opq16.search_refine(good, c.q, 3, 10, nprobe=0)          # the exhaustive scan needs coarseK == 1
    assert err.value.code == CVTMI_EINVAL
    d, i = opq1.search_refine(good, c.q, 3, 10)
    assert (i >= 0).all()
    for ix in (opq1, opq16, good, wrong_d, wrong_n, wrong_m):
        ix.close()
