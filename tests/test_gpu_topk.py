"""GPU: the selection kernel on its own -- topk_merge_kernel (csrc/topk_merge.hip) over the LDS selection of block_topk.h, through
its three public entries: cvtmi_topk_select[_dev] (get_sort_results), cvtmi_topk_merge[_dev] and the GATHERED merge behind
cvtmi_shard_merge_topk_dev.  Expected = a numpy model of the documented order: a stable sort on (key, position) where the key is
the f32_key total order with -0.0 taken as +0.0 and 0x7fffffff keyed as 0x7ffffffe; k entries, padding (+inf, -1).  Ids and
distance bits must match exactly (a returned -0.0 keeps its sign: the kernel re-reads its input).  Where no NaN is involved the
CPU oracle's (float, id) pair order is checked as well.

The sizes sit at the edges of the 1024-candidate tiles and of both buffer variants (CAP 1024 / TRIG 768 for k <= 384, CAP 4096 /
TRIG 3072 above); the patterns force the overflow retry (strictly descending rows), the '<' fast path against copies of the k-th
value, ties across tile boundaries, signed zeros, infinities, denormals and NaNs of both signs."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

INF_BITS = 0x7F800000
KS = (1, 2, 64, 100, 128, 129, 383, 384, 385, 1000, 2047, 2048)
PATTERNS = ("random", "ascending", "descending", "equal", "small_ints", "best_last", "best_first_then_kth", "runs", "zeros",
            "specials", "nan")


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()
    return cvt_amd


def f32(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def dev_keys(d):
    """The kernel's key of every distance (uint32): f32_key with -0.0 as +0.0, KEY_MAX kept free."""
    u = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    k = np.where((u >> 31) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[k == 0xFFFFFFFF] = 0xFFFFFFFE
    return k


def model_pick(d, valid, k):
    """positions of the k smallest (key, position) among the valid candidates of one query"""
    pos = np.flatnonzero(valid)
    o = pos[np.argsort(dev_keys(d[pos]), kind="stable")]
    return o[:k]


def model_select(rows, k):
    nq, n = rows.shape
    od = np.full((nq, k), f32(INF_BITS), np.float32)
    oi = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        o = model_pick(rows[q], np.ones(n, bool), k)
        od[q, :o.size] = rows[q][o]
        oi[q, :o.size] = o
    return od, oi


def model_merge(in_d, in_i, k):
    """in_d / in_i [nq][L][k]: candidate position = l * k + j, ids < 0 are padding"""
    nq = in_d.shape[0]
    od = np.full((nq, k), f32(INF_BITS), np.float32)
    oi = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        d, i = in_d[q].reshape(-1), in_i[q].reshape(-1)
        o = model_pick(d, i >= 0, k)
        od[q, :o.size] = d[o]
        oi[q, :o.size] = i[o]
    return od, oi


def same(got, want, ctx):
    gd, gi = (np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in got)
    wd, wi = want
    assert gi.shape == wi.shape, ctx
    bad = np.flatnonzero((gi != wi).any(axis=1) | (bits(gd) != bits(wd)).any(axis=1))
    if bad.size:
        q = int(bad[0])
        j = int(np.flatnonzero((gi[q] != wi[q]) | (bits(gd[q]) != bits(wd[q])))[0])
        raise AssertionError("%s: row %d, first difference at %d: got (%08x, %d), want (%08x, %d)" % (
            ctx, q, j, int(bits(gd[q, j:j + 1])[0]), gi[q, j], int(bits(wd[q, j:j + 1])[0]), wi[q, j]))


def pattern(name, n, k, rng):
    if n == 0:
        return np.zeros(0, np.float32)
    pos = np.arange(n)
    if name == "random":
        return rng.normal(size=n).astype(np.float32)
    if name == "ascending":
        return np.sort(rng.normal(size=n)).astype(np.float32)
    if name == "descending":                   # every tile beats the threshold: overflow + '<=' retry for k <= 384
        return (n - pos).astype(np.float32) * np.float32(0.5)
    if name == "equal":
        return np.full(n, 2.5, np.float32)
    if name == "small_ints":                   # mass ties
        return rng.integers(-2, 3, size=n).astype(np.float32)
    if name == "best_last":                    # the k smallest in the last tile
        x = rng.uniform(10, 20, size=n).astype(np.float32)
        m = min(k, n)
        x[n - m:] = rng.uniform(0, 1, size=m).astype(np.float32)
        return x
    if name == "best_first_then_kth":          # k best first, then only copies of the k-th value: nothing may displace them
        m = min(k, n)
        x = np.empty(n, np.float32)
        x[:m] = rng.permutation(np.arange(m, dtype=np.float32))
        x[m:] = np.float32(m - 1)
        return x
    if name == "runs":                         # descending runs of equal values that straddle the 1024-candidate tiles
        return ((n - 1 - pos) // 300).astype(np.float32)
    if name == "zeros":                        # +0 / -0 interleaved, a few values on either side
        x = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        x[pos % 7 == 3] = 1.0
        x[pos % 11 == 5] = -1.0
        return x
    if name == "specials":
        pool = np.array([np.inf, -np.inf, 0.0, -0.0, 3.4028235e38, -3.4028235e38, 1e-45, -1e-45, 1e-40, -1e-40,
                         1.1754942e-38, 1.0, -1.0], np.float32)
        return pool[rng.integers(0, pool.size, size=n)]
    if name == "nan":
        x = rng.normal(size=n).astype(np.float32)
        nans = f32([0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0x7FFFFFFE, 0xFFFFFFFF, 0x7F800001, 0xFF800001])
        sel = rng.random(n) < 0.2
        x[sel] = nans[rng.integers(0, nans.size, size=int(sel.sum()))]
        x[pos % 13 == 0] = np.inf
        x[pos % 17 == 0] = -np.inf
        return x
    raise ValueError(name)


def sizes_for(k):
    s = {0, 1, k - 1, k, k + 1, 767, 768, 769, 1023, 1024, 1025, 3071, 3072, 3073, 4096, 4097}
    if k in (1, 128, 384, 385, 2048):
        s.add(100_003)
    return sorted(v for v in s if v >= 0)


def select_both(amd, rows, k):
    """host entry and device entry (torch tensors on a side stream)"""
    import torch
    h = amd.topk_select(rows, k)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.from_numpy(rows).cuda()
        dd, di = amd.topk_select(t, k)
        d_np, i_np = dd.cpu().numpy(), di.cpu().numpy()
    s.synchronize()
    return h, (d_np, i_np)


def oracle_check(orc, rows, got, k, names):
    """the CPU oracle's pair order (qsort on (float, index)) on the rows without NaN"""
    gd, gi = got
    for q, name in enumerate(names):
        if name == "nan" or rows.shape[1] == 0:
            continue
        od, oi = orc.topk_pairs(rows[q], k)
        m = od.size
        assert np.array_equal(gi[q, :m], oi) and np.array_equal(bits(gd[q, :m]), bits(od)), (name, k, rows.shape[1])
        assert np.all(gi[q, m:] == -1) and np.all(bits(gd[q, m:]) == INF_BITS)


@pytest.mark.parametrize("k", KS)
def test_topk_select_edges(amd, orc, k):
    """every size edge of both buffer variants, nq = 11 rows of which each holds another pattern"""
    rng = np.random.default_rng(1000 + k)
    for n in sizes_for(k):
        rows = np.stack([pattern(p, n, k, rng) for p in PATTERNS]) if n else np.zeros((len(PATTERNS), 0), np.float32)
        rows = np.ascontiguousarray(rows, np.float32)
        want = model_select(rows, k)
        h, dv = select_both(amd, rows, k)
        same(h, want, "host k=%d n=%d" % (k, n))
        same(dv, want, "device k=%d n=%d" % (k, n))
        oracle_check(orc, rows, h, k, PATTERNS)


@pytest.mark.parametrize("k", (4, 100, 1000))
def test_topk_select_signed_zero_by_index(amd, k):
    """{+0, -0, +0, -0, ...}: the reference's pairs tie the two zeros and go by index, and each output keeps its own sign"""
    n = max(4, 2 * k)
    row = np.where(np.arange(n) % 2 == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)[None, :]
    for got in select_both(amd, row, k):
        gd, gi = got
        assert np.array_equal(gi[0], np.arange(k)), gi[0][:8]
        assert np.array_equal(bits(gd[0]), np.where(np.arange(k) % 2 == 1, 0x80000000, 0).astype(np.uint32))


def test_topk_select_nan_order(amd):
    """{3, 1, NaN, 2, 0.5, 4} and a NaN of each sign: -NaN before -inf, +NaN after +inf, 0x7fffffff tied with 0x7ffffffe"""
    row = np.array([3, 1, np.nan, 2, 0.5, 4], np.float32)[None, :]
    for gd, gi in select_both(amd, row, 3):
        assert gi[0].tolist() == [4, 1, 3]
    row = f32([0x7FC00000, 0xFF800000, 0x7FFFFFFF, 0xFFC00000, 0x7F800000, 0x7FFFFFFE, 0x3F800000])[None, :]
    for gd, gi in select_both(amd, row, 7):
        assert gi[0].tolist() == [3, 1, 6, 4, 0, 2, 5]
        assert np.array_equal(bits(gd[0]), bits(row[0][[3, 1, 6, 4, 0, 2, 5]]))


def test_topk_select_two_million(amd):
    """a couple of queries over ~2 M scores: random, strictly descending (a retry in every tile for k <= 384), tie runs"""
    import torch
    rng = np.random.default_rng(77)
    n = 2_000_003
    rows = np.stack([pattern("random", n, 1, rng), pattern("descending", n, 1, rng), pattern("runs", n, 1, rng)])
    t = torch.from_numpy(rows).cuda()
    for k in (100, 384, 385, 2048):
        want = model_select(rows, k)
        same(amd.topk_select(t, k), want, "2M k=%d" % k)
    same(amd.topk_select(rows[1:2], 384), model_select(rows[1:2], 384), "2M host")


def test_topk_select_argument_errors(amd):
    """k = 0 / k > CVTMI_K_MAX are refused with their codes; nq = 0 is a no-op that touches nothing"""
    import torch
    lib = amd.lib()
    x = np.ones((2, 10), np.float32)
    d = np.full((2, 2049), 7.0, np.float32); i = np.full((2, 2049), 7, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.cvtmi_topk_select(p(x), C.c_int64(2), C.c_int64(10), C.c_int(0), p(d), p(i)) == -1          # CVTMI_EINVAL
    assert lib.cvtmi_topk_select(p(x), C.c_int64(2), C.c_int64(10), C.c_int(2049), p(d), p(i)) == -5       # CVTMI_EUNSUPPORTED
    assert lib.cvtmi_topk_select(p(x), C.c_int64(0), C.c_int64(10), C.c_int(5), p(d), p(i)) == 0
    assert np.all(d == 7.0) and np.all(i == 7)
    t = torch.from_numpy(x).cuda()
    od = torch.empty((2, 2049), dtype=torch.float32, device="cuda"); oi = torch.empty((2, 2049), dtype=torch.int64, device="cuda")
    tp = lambda a: C.c_void_p(a.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.cvtmi_topk_select_dev(tp(t), C.c_int64(2), C.c_int64(10), C.c_int(0), tp(od), tp(oi), st) == -5
    assert lib.cvtmi_topk_select_dev(tp(t), C.c_int64(2), C.c_int64(10), C.c_int(2049), tp(od), tp(oi), st) == -5
    assert lib.cvtmi_topk_select_dev(None, C.c_int64(0), C.c_int64(10), C.c_int(5), None, None, st) == 0
    with pytest.raises(amd.CvtmiError):
        amd.topk_select(t, 2049)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# merge
# ---------------------------------------------------------------------------------------------------------------------------
def make_lists(rng, nq, L, k, span=1_000_000, kind="mixed"):
    """L lists per query, list l holding ids of [l * span, (l + 1) * span), each sorted by (key, id); padded tails, +inf with
    real ids, ties inside and across lists, +0 in lower lists against -0 in higher ones"""
    d = np.empty((nq, L, k), np.float32)
    ids = np.empty((nq, L, k), np.int64)
    for q in range(nq):
        for l in range(L):
            if kind == "nan":
                v = pattern("nan", k, k, rng)
            else:
                v = rng.integers(1, 4, size=k).astype(np.float32)
                v[rng.random(k) < 0.4] = np.float32(-0.0) if l % 2 else np.float32(0.0)   # +0 in even lists, -0 in odd ones
                if q % 2 == 0:
                    v[rng.random(k) < 0.1] = -0.0
                neg = rng.random(k) < 0.5 / L                                   # ~k / 2 negatives in all: zeros fill the rest of the top k
                v[neg] = -rng.integers(1, 3, size=int(neg.sum())).astype(np.float32)
                v[rng.random(k) < 0.05] = np.inf                                # real ids at +inf: ahead of any padding
            i = l * span + np.cumsum(rng.integers(1, 100, size=k))             # distinct, ascending, inside the list's range
            o = np.lexsort((i, dev_keys(v)))
            d[q, l], ids[q, l] = v[o], i[o]
            pad = int(rng.integers(0, k + 1)) if (q + l) % 3 == 0 else 0         # padded tail: (+inf, -1)
            if pad:
                d[q, l, k - pad:] = np.inf
                ids[q, l, k - pad:] = -1
    return d, ids


@pytest.mark.parametrize("L", (1, 2, 7, 64))
@pytest.mark.parametrize("k", (1, 5, 100, 384, 385, 1000, 2048))
def test_topk_merge_lists(amd, orc, L, k):
    import torch
    rng = np.random.default_rng(L * 4099 + k)
    nq = 4
    d, ids = make_lists(rng, nq, L, k)
    want = model_merge(d, ids, k)
    same(amd.topk_merge(d, ids, k), want, "merge host L=%d k=%d" % (L, k))
    same(orc.merge_topk(d, ids, k), want, "oracle L=%d k=%d" % (L, k))     # the (float, id) pair order agrees with the model
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = amd.topk_merge(torch.from_numpy(d).cuda(), torch.from_numpy(ids).cuda(), k)
        got = (got[0].cpu().numpy(), got[1].cpu().numpy())
    s.synchronize()
    same(got, want, "merge device L=%d k=%d" % (L, k))
    dn, idn = make_lists(rng, 2, L, k, kind="nan")
    same(amd.topk_merge(dn, idn, k), model_merge(dn, idn, k), "merge NaN L=%d k=%d" % (L, k))


def test_topk_merge_signed_zero_across_lists(amd):
    """+0 in the lower-id list against -0 in the higher-id one: the pairs are equal, the lower id goes first"""
    k = 4
    d = np.array([[[0.0, 0.0, 1, 1], [-0.0, -0.0, -0.0, 1]]], np.float32)
    ids = np.array([[[0, 1, 2, 3], [10, 11, 12, 13]]], np.int64)
    gd, gi = amd.topk_merge(d, ids, k)
    assert gi[0].tolist() == [0, 1, 10, 11]
    assert bits(gd[0]).tolist() == [0, 0, 0x80000000, 0x80000000]


@pytest.mark.parametrize("k", (3, 100, 385, 2048))
def test_topk_merge_uint8_distances(amd, k):
    """uint8-L2 lists send int32 distances as their bit patterns (0 ... 300 are fp32 denormals): integer order, bits untouched"""
    rng = np.random.default_rng(k)
    nq, L = 3, 7
    di = np.sort(rng.integers(0, 301, size=(nq, L, k)), axis=2).astype(np.int32)
    ids = np.empty((nq, L, k), np.int64)
    for l in range(L):
        ids[:, l] = l * 10_000 + np.arange(k)
    ids[1, 3, k // 2:] = -1
    d = di.view(np.float32)
    gd, gi = amd.topk_merge(d, ids, k)
    want = model_merge(d, ids, k)
    same((gd, gi), want, "uint8 k=%d" % k)
    flat_d, flat_i = di.reshape(nq, -1), ids.reshape(nq, -1)
    for q in range(nq):
        ok = flat_i[q] >= 0
        o = np.lexsort((flat_i[q][ok], flat_d[q][ok]))[:k]
        assert np.array_equal(gd[q].view(np.int32)[:o.size], flat_d[q][ok][o]) and np.array_equal(gi[q][:o.size], flat_i[q][ok][o])


# ---------------------------------------------------------------------------------------------------------------------------
# gathered merge (cvtmi_shard_merge_topk_dev): rank 0 of W, the other ranks' slots written by the all-gather callback
# ---------------------------------------------------------------------------------------------------------------------------
def _align16(b):
    return (b + 15) // 16 * 16


@pytest.mark.parametrize("W", (1, 3))
@pytest.mark.parametrize("k", (1, 384, 385, 2048))
def test_gathered_merge(amd, W, k):
    import torch
    rng = np.random.default_rng(W * 31 + k)
    nq = 5
    d, ids = make_lists(rng, nq, W, k, span=1 << 40)
    for q in range(nq):                                  # a signed-zero tie across every pair of ranks
        for r in range(W):
            d[q, r, 0] = np.float32(-0.0) if r % 2 else np.float32(0.0)
            ids[q, r, 0] = r * (1 << 40) + 5
            o = np.lexsort((np.where(ids[q, r] < 0, np.iinfo(np.int64).max, ids[q, r]), dev_keys(d[q, r])))
            d[q, r], ids[q, r] = d[q, r][o], ids[q, r][o]
    want = model_merge(d, ids, k)
    fd, fi = nq * k * 4, nq * k * 8
    slot = 16 + _align16(fd) + _align16(fi)
    blobs = []
    for r in range(W):                                   # [status word, 16 B][distances, 16 B-aligned][ids, 16 B-aligned]
        b = np.zeros(slot, np.uint8)
        b[16:16 + fd] = np.ascontiguousarray(d[:, r]).view(np.uint8).reshape(-1)
        b[16 + _align16(fd):16 + _align16(fd) + fi] = np.ascontiguousarray(ids[:, r]).view(np.uint8).reshape(-1)
        blobs.append(b)
    calls = []
    hip = C.CDLL("libamdhip64.so")

    def gather(send, recv, nbytes, stream):
        calls.append(nbytes)
        assert nbytes == slot and send == recv, (nbytes, slot)
        torch.cuda.current_stream().synchronize()
        for r in range(1, W):
            if hip.hipMemcpy(C.c_void_p(recv + r * nbytes), C.c_void_p(blobs[r].ctypes.data), C.c_size_t(nbytes), C.c_int(1)) != 0:
                return 1
        return 0

    comm = amd.Comm.custom(gather, 0, W)
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            ld = torch.from_numpy(np.ascontiguousarray(d[:, 0])).cuda()
            li = torch.from_numpy(np.ascontiguousarray(ids[:, 0])).cuda()
            od, oi = comm.merge_topk(ld, li, k)
            got = (od.cpu().numpy(), oi.cpu().numpy())
        s.synchronize()
        comm.status()
    finally:
        comm.close()
    if W > 1:
        assert len(calls) == 1
    same(got, want, "gathered W=%d k=%d" % (W, k))
