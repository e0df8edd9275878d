"""GPU parity of the fp32 threshold filter (flat_f32_tfilter.hip) and the fp32 stream (flat_f32_stream.hip) on data built against their
proofs, not random data: rows tied to within the margin around each query's k-th score (the margin's derivation), tables whose sample
cannot fill k slots (the k-th sample maximum), and queries whose buffer is followed by garbage (the per-query margin terms).

Every case compares the lists and the distance bits with the checker (the reference's own summation order) and asserts the route it
targets and how many queries the exact kernels re-answered (cvtmi_flat_last_redo): a case cannot pass because the filter gave up."""
import concurrent.futures as cf
import os

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu
IP, L2F, L2U8 = 0, 1, 2
MARGIN0 = 2.0 ** -13   # the margin's smallest fixed term, in units of Q = |q|^2 + max |x|^2


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()
    cvt_amd.set_tuning("flat_count_redo", 1)
    yield cvt_amd
    cvt_amd.set_tuning("flat_count_redo", 0)


def _oracle(orc, metric, x, q, k):
    """the checker on every query, the queries split over threads (each call is one C loop that releases the GIL)"""
    flavour = 4 if metric == IP else 8
    parts = max(1, min(len(q), int(os.environ.get("OMP_NUM_THREADS", 16))))
    chunks = [c for c in np.array_split(np.arange(len(q)), parts) if len(c)]
    with cf.ThreadPoolExecutor(len(chunks)) as ex:
        res = list(ex.map(lambda c: orc.flat_search(metric, x, q[c], k, flavour=flavour), chunks))
    return np.concatenate([r[0] for r in res]), np.concatenate([r[2] for r in res])


def _same(ds, is_, od, oi, what):
    ds = np.asarray(ds); is_ = np.asarray(is_)
    bad = np.nonzero(~(np.all(is_ == oi, axis=1) & np.all(bits(ds) == bits(od), axis=1)))[0]
    assert len(bad) == 0, "%s: %d queries differ from the checker, first %s" % (what, len(bad), bad[:8])


def _bf16(a):
    """a rounded to bf16 (nearest even), as float32"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def _bf16_ulp_step(v, up):
    """v (bf16-exact, positive) moved by one bf16 unit in the last place"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.int64)
    u = u + np.where(up, 0x10000, -0x10000)
    return u.astype(np.uint32).view(np.float32)


def _scores(metric, x, q):
    """T = x.q + b_x in float64 (b_x = -|x|^2 / 2 for L2): larger is nearer"""
    x64 = x.astype(np.float64); q64 = q.astype(np.float64)
    t = q64 @ x64.T
    if metric == L2F:
        t -= 0.5 * np.einsum("ij,ij->i", x64, x64)[None, :]
    return t


def _positive_mixed(rng, shape):
    """same-sign bf16-exact values over six binades: the partial sums of a dot product round at every step"""
    return _bf16(np.ldexp(1.0 + rng.random(shape), -rng.integers(0, 6, shape)).astype(np.float32))


def _near_tie_table(rng, metric, n, D, nq, group):
    """bf16-exact rows and queries (the operands' split residues are zero: the fixed term is the whole margin).  Query j owns `group`
    rows scattered over the table: one-ulp perturbations of a base row in one to three coordinates (its smaller entries) and exact
    duplicates of it -- its k best for every k up to ~group sit within a fraction of the margin of each other"""
    x = _positive_mixed(rng, (n, D))
    q = _positive_mixed(rng, (nq, D))
    where = rng.permutation(n)[:nq * group].reshape(nq, group)
    for j in range(nq):
        base = q[j] * np.float32(2.0 if metric == IP else 1.0)   # (exact: a power of two)
        small = np.argsort(base)[:max(4, D // 4)]
        g = np.repeat(base[None, :], group, axis=0)
        for r in range(group):
            if r % 8 == 0:
                continue                                          # an exact duplicate
            cols = rng.choice(small, size=1 + r % 3, replace=False)
            g[r, cols] = _bf16_ulp_step(g[r, cols], rng.random(len(cols)) < 0.5)
        x[where[j]] = g
    return np.ascontiguousarray(x), np.ascontiguousarray(q)


def _band_check(metric, x, q, ks, want=50):
    """the data's own claim: each query has `want` rows or more within the smallest margin of its k-th score"""
    t = _scores(metric, x, q)
    Qb = np.einsum("ij,ij->i", q.astype(np.float64), q.astype(np.float64)) + np.max(np.einsum("ij,ij->i", x.astype(np.float64), x.astype(np.float64)))
    ts = -np.sort(-t, axis=1)
    for k in ks:
        tk = ts[:, k - 1]
        inband = np.sum(np.abs(t - tk[:, None]) <= MARGIN0 * Qb[:, None], axis=1)
        assert inband.min() >= want, (k, inband.min())


@pytest.mark.parametrize("metric", [IP, L2F])
@pytest.mark.parametrize("D,prods", [(128, 3), (256, 1), (256, 2), (300, 1), (1024, 1), (1200, 1), (1536, 1), (2048, 1)])
def test_tfilter_wide_row_near_ties(amd, orc, metric, D, prods):
    """rows tied to within the margin around the k-th score at every width class (128-d with three products as the control; 256-d
    with one and two; 300 ... 2048-d with one, 1536 / 2048-d in two K halves).  The margin's fixed term must cover the accumulation
    of every product term and the reference's own rounding at width D: too small a margin drops a true neighbour silently"""
    rng = np.random.default_rng(D * 10 + prods + 7 * metric)
    n, nq, ks = 40_000 + 13, 32, (1, 10, 100)
    x, q = _near_tie_table(rng, metric, n, D, nq, 200)
    _band_check(metric, x, q, ks)
    od, oi = _oracle(orc, metric, x, q, max(ks))
    try:
        amd.set_tuning("flat_f32_tfilter", prods); amd.set_tuning("flat_f32_tfilter_min", 16); amd.set_tuning("flat_f32_tfilter_min_rows", 32768)
        ix = amd.FlatIndex(metric, D); ix.add(x)
        for k in ks:
            ds, is_ = ix.search(q, k)
            assert ix.last_search()[0] == 3, k
            assert ix.last_redo() == 0, k
            _same(ds, is_, od[:, :k], oi[:, :k], "k=%d" % k)
        ix.close()
    finally:
        amd.set_tuning("flat_f32_tfilter", 4); amd.set_tuning("flat_f32_tfilter_min", 0); amd.set_tuning("flat_f32_tfilter_min_rows", 262144)


def _cluster_table(rng, metric, n, D, nq, high=3000, bases=30):
    """queries around one direction; `high` rows clustered just above the rest for every query, perturbations of `bases` base rows
    (near ties at the k-th place for k = 1537 ... 2048), spread over the table"""
    c = np.abs(rng.normal(size=D)).astype(np.float32) + 0.5
    q = (c[None, :] + 0.01 * rng.normal(size=(nq, D))).astype(np.float32)
    x = (0.6 * c[None, :] + 0.3 * rng.normal(size=(n, D))).astype(np.float32)
    b = (c[None, :] * (1.3 if metric == IP else 1.0) + 0.05 * rng.normal(size=(bases, D))).astype(np.float32)
    h = b[rng.integers(0, bases, high)] + (1e-4 * rng.normal(size=(high, D))).astype(np.float32)
    h[::7] = b[rng.integers(0, bases, len(h[::7]))]   # exact duplicates of the bases
    x[rng.permutation(n)[:high]] = h
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(q, np.float32)


def _ft_filled_slots(D, n, k):
    """sample slots the fp32 threshold filter fills for k = 129 .. 2048 on n rows (one query chunk; the products the dispatch takes): the
    whole table is the sample below ~260 K rows at D <= 32 -- two slots per tile group of 128 rows"""
    nch = 2 if D <= 32 else 4
    rt = (4 if nch == 2 else 3) if k > 768 else 4 if nch <= 4 else 3
    groups = (-(-n // 32) + rt - 1) // rt
    sample = max(groups // 3, min(groups, -(-2048 // rt)))
    sample = min(groups, max(1, (sample + 1024) // 2048) * 2048)
    return 2 * min(sample, 2048)


@pytest.mark.parametrize("metric,D,n,k,nq", [
    (L2F, 32, 98_304, 1537, 40),      # 1536 slots: fewer than k
    (IP, 32, 100_000, 1600, 256),     # 1564 slots: fewer than k
    (L2F, 16, 100_000, 2048, 1),
    (L2F, 64, 100_000, 2048, 1),      # 2084 slots: k of them, not 1.25 k
    (IP, 32, 131_071, 2048, 40),      # 2048 slots: exactly k
    (L2F, 64, 100_000, 1600, 40),     # 2084 slots >= 1.25 k: just inside the rule
    (L2F, 32, 131_071, 1537, 256),    # 2048 slots >= 1.25 k: just inside
    (IP, 64, 400_000, 2048, 40),      # a third of the table: 4096 slots
    (L2F, 16, 400_000, 1600, 1),
])
def test_tfilter_sample_shortage(amd, orc, metric, D, n, k, nq):
    """k = 1537 ... 2048 on tables of 98 304 ... 400 000 rows, where the sample's 4096 slots are only partly filled: theta must be the
    k-th largest of k filled slots.  A shape with fewer than 1.25 k filled slots leaves the threshold filter (the exact kernels answer
    it whole); a shape inside the rule is answered by the filter without a single query handed back"""
    rng = np.random.default_rng(n + k + D + nq + metric)
    x, q = _cluster_table(rng, metric, n, D, nq)
    od, oi = _oracle(orc, metric, x, q, k)
    ix = amd.FlatIndex(metric, D); ix.add(x)
    ds, is_ = ix.search(q, k)
    route, redo = ix.last_search()[0], ix.last_redo()
    ix.close()
    _same(ds, is_, od, oi, "route %d" % route)
    inside = 4 * _ft_filled_slots(D, n, k) >= 5 * k
    if inside:
        assert route == 3 and redo == 0, (route, redo)
    else:
        assert route != 3, (route, redo)


@pytest.mark.parametrize("n,inside", [(128_000, True), (127_872, False)])
def test_u8_tfilter_sample_boundary(amd, orc, n, inside):
    """the uint8 threshold filter at its own sample rule (k = 1600 over 64-byte rows: 1000 tile groups of 128 rows fill 2000 = 1.25 k
    slots, 999 do not) -- it shares the k-th-slot selection with the fp32 filter"""
    rng = np.random.default_rng(n)
    D, k, nq = 64, 1600, 40
    c = rng.integers(60, 200, D)
    x = np.clip(c[None, :] + rng.integers(-50, 51, (n, D)), 0, 255).astype(np.uint8)
    hi = np.clip(c[None, :] + rng.integers(-3, 4, (3000, D)), 0, 255).astype(np.uint8)
    x[rng.permutation(n)[:3000]] = hi
    q = np.clip(c[None, :] + rng.integers(-2, 3, (nq, D)), 0, 255).astype(np.uint8)
    _, odi, oi = orc.flat_search(L2U8, x, q, k)
    ix = amd.FlatIndex(L2U8, D); ix.add(x)
    d, i = ix.search(q, k)
    route, redo = ix.last_search()[0], ix.last_redo()
    ix.close()
    assert np.array_equal(i, oi) and np.array_equal(d, odi)
    if inside:
        assert route == 4 and redo == 0, (route, redo)
    else:
        assert route != 4, route


@pytest.mark.parametrize("metric", [IP, L2F])
@pytest.mark.parametrize("D", [20, 36, 100, 300, 900])
def test_tfilter_query_tail(amd, orc, metric, D):
    """D % 8 == 4: the query's last eight-float piece ends four floats past the query.  The queries as a view of the first nq D floats of
    a larger device tensor whose next four floats are NaN, Inf or 1e30 (inside the same allocation): lists, bits and the count of
    queries handed to the exact kernels must equal those of the same queries without a tail"""
    import torch
    rng = np.random.default_rng(D * 3 + metric)
    n = 33_000 + 7
    x = rng.normal(size=(n, D)).astype(np.float32)
    if metric == IP:
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    try:
        amd.set_tuning("flat_f32_tfilter_min_rows", 32768)
        ix = amd.FlatIndex(metric, D); ix.add(x)
        for nq in (16, 129, 1000):
            k = 10 if nq == 1000 else 32
            q = (x[rng.integers(0, n, nq)] + 0.1 * rng.normal(size=(nq, D))).astype(np.float32)
            def tailed(junk):   # the queries, then four floats of junk, inside one allocation
                buf = torch.zeros(nq * D + 256, dtype=torch.float32, device="cuda")
                buf[:nq * D] = torch.from_numpy(q).cuda().reshape(-1)
                buf[nq * D:nq * D + 4] = junk
                return buf, buf[:nq * D].view(nq, D)
            _, clean = tailed(0.0)
            d0, i0 = ix.search(clean, k)
            torch.cuda.synchronize()
            route0, redo0 = ix.last_search()[0], ix.last_redo()
            assert route0 == 3, nq
            d0 = d0.cpu().numpy(); i0 = i0.cpu().numpy()
            for junk in (float("nan"), float("inf"), 1e30):
                buf, qv = tailed(junk)
                d1, i1 = ix.search(qv, k)
                torch.cuda.synchronize()
                assert ix.last_search()[0] == 3, (nq, junk)
                assert ix.last_redo() == redo0, (nq, junk, ix.last_redo(), redo0)
                assert np.array_equal(i1.cpu().numpy(), i0) and np.array_equal(bits(d1.cpu().numpy()), bits(d0)), (nq, junk)
            # the checker on every query of the small batches; the large one on its last 32 (the query the tail follows)
            sel = np.arange(nq) if nq <= 129 else np.arange(nq - 32, nq)
            od, oi = _oracle(orc, metric, x, q[sel], k)
            _same(d0[sel], i0[sel], od, oi, "nq=%d" % nq)
            assert redo0 == 0, (nq, redo0)
        ix.close()
    finally:
        amd.set_tuning("flat_f32_tfilter_min_rows", 262144)


@pytest.mark.parametrize("metric,D", [(IP, 64), (L2F, 128)])
def test_stream_near_ties(amd, orc, metric, D):
    """the fp32 stream (route 2; the four-wave shared ring: more queries than one wave's private ring takes) on the near-tie table: its
    margin, its first threshold from the k-th of 1024 wave maxima and its finish's selection are the same code as the filter's"""
    rng = np.random.default_rng(D + metric)
    n, nq, ks = 100_000 + 21, 300, (1, 10, 100)
    x, q = _near_tie_table(rng, metric, n, D, nq, 160)
    _band_check(metric, x, q, ks)
    od, oi = _oracle(orc, metric, x, q, max(ks))
    try:
        amd.set_tuning("flat_f32_tfilter", 0); amd.set_tuning("flat_f32_share", 1)
        ix = amd.FlatIndex(metric, D); ix.add(x)
        for k in ks:
            ds, is_ = ix.search(q, k)
            assert ix.last_search()[0] == 2, k
            assert ix.last_redo() == 0, k
            _same(ds, is_, od[:, :k], oi[:, :k], "k=%d" % k)
        ix.close()
    finally:
        amd.set_tuning("flat_f32_tfilter", 4); amd.set_tuning("flat_f32_share", 0)
