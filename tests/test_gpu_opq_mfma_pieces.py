"""The "scan_mfma" route (cvt_amd/csrc/adc_mfma.hip over the filter kernels of flat_u8_tfilter.hip) where the headline search runs it and
the other route files do not: batches that go through in more than one piece (launch_adc_mfma's loop with q0 > 0: everything of a later
piece is indexed inside the piece AND inside the call, in scratch the piece before left full), pieces of three chunks and more (spx 8,
mf_theta_kernel<16>, chunks of 192 / 224 queries, a last chunk that ends inside a query block), the widths D = 32 / 96 / 256 on this
caller (bias_direct, int8 rows of mf_pack_kernel), and a record region that runs over.  Against the oracle and against the scan the route
stands in front of: ids with np.array_equal, distances by bit pattern.  Every case asserts the plan it is about (cvtmi_opq_mfma_plan: queries
per piece, pieces; the same figures are pinned on the CPU in test_adc_mfma_plan.py) before it searches, and that the route, not the scan
behind it, answered: all queries on the route and fewer than an eighth of them flagged, unless the case is about flagged queries."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

D, M, K = 128, 16, 256
ROWS, NQ, SMALL, TINY = 20000, 3100, 8192 + 37, 97
BASE = 5_000_000_000


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()
    return cvt_amd


def _make_world(amd, orc, d, rows, nq, seed_r, seed_x):
    """a rotation, codebooks trained on 8192 rotated SIFT-like rows, `rows` encoded rows and nq distinct queries of width d"""
    from cvt_amd import synth
    w = type("World", (), {})()
    w.D = d
    # (the dense rotation is built for widths up to 128: a wider model is a permutation model, whose rotation is exact -- the library's own)
    w.rot = {"R": synth.random_rotation(d, seed=seed_r)} if d <= 128 else {"perm": synth.random_permutation(d, seed=seed_r)}
    x = synth.sift_like(rows, d, seed=seed_x, device="cuda")
    probe = amd.OpqIndex(np.zeros((1, d), np.float32), np.zeros((M, K, d // M), np.float32), **w.rot)
    w.books = synth.train_books(probe.rotate(x[:8192]), M, K, iters=2).astype(np.float32)
    probe.close()
    enc = amd.OpqIndex(np.zeros((1, d), np.float32), w.books, **w.rot)
    _, codes = enc.rotate_encode(x)
    w.codes = codes.cpu().numpy()
    w.q = synth.sift_like(nq, d, seed=0xBEEF, device="cuda").cpu().numpy()
    # (a result written to the wrong query of another piece must not be able to match)
    assert len(np.unique(w.q, axis=0)) == nq
    w.q_rot = orc.rotate_fma(w.rot["R"], w.q) if "R" in w.rot else enc.rotate(w.q)
    enc.close()
    w.memo = {}
    return w


@pytest.fixture(scope="module")
def world(amd, orc):
    """D = 128: 20 000 encoded rows, 3100 queries; shared by the cases, never written"""
    return _make_world(amd, orc, D, ROWS, NQ, 11, 0xC0DE)


_WIDTHS = {}


def _width_world(amd, orc, d):
    if d not in _WIDTHS:
        _WIDTHS[d] = _make_world(amd, orc, d, SMALL, 1700 if d == 96 else 600, 3 + d, 0xD00 + d)
    return _WIDTHS[d]


def _plan(d, n, nq, k, cap=4096, sample=2):
    import cvt_amd
    out = (C.c_int64 * 3)()
    rc = cvt_amd.lib().cvtmi_opq_mfma_plan(C.c_int(d), C.c_int64(n), C.c_int64(nq), C.c_int(k), C.c_int(cap), C.c_int(sample), out)
    assert rc == 0, (d, n, nq, k, cap, sample)
    return int(out[0]), int(out[1])


def _layout(m):
    """(chunks, queries per chunk, row slices per chunk and XCD) of a piece of m queries: mf_shape's rule"""
    chunks = (m + 255) // 256
    qper = ((m + chunks - 1) // chunks + 31) // 32 * 32
    return chunks, qper, 32 if chunks == 1 else (16 if chunks == 2 else 8)


def _index(amd, w, codes, **params):
    idx = amd.OpqIndex(np.zeros((1, w.D), np.float32), w.books, **w.rot)
    idx.add_codes(codes)
    for name, v in (("scan_mfma_min_nq", 1), ("scan_mfma_min_rows", 1), ("profile", 1)) + tuple(params.items()):
        idx.set_param(name, v)
    return idx


def _oracle(orc, w, n, k):
    """the oracle's answer for ALL of the world's queries over its first n rows, once per (n, k)"""
    if (n, k) not in w.memo:
        w.memo[(n, k)] = orc.adc_search(w.q_rot, w.books, w.codes[:n], k)
    return w.memo[(n, k)]


def _same(d, i, od, oi, skip=()):
    return [f for f in range(d.shape[0]) if f not in skip and not (np.array_equal(i[f], oi[f]) and np.array_equal(bits(d[f]), bits(od[f])))]


def _where(bad, per):
    """failing queries as (query, piece, index inside the piece): an off-by-piece error reads as one"""
    return [(f, f // per, f % per) for f in bad[:8]]


def _search_both(idx, q, k):
    """(answer of the route, its (queries, flagged), answer of the scan)"""
    import torch
    qd = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    idx.set_param("scan_mfma", 1)
    got = idx.search(qd, k)
    stat = idx.last_mfma()
    idx.set_param("scan_mfma", 0)
    ref = idx.search(qd, k)
    idx.set_param("scan_mfma", 1)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in got), stat, tuple(t.cpu().numpy() for t in ref)


def _check(idx, q, k, od, oi, what, per, flagged="few", skip=()):
    """one search of q on the route and one on the scan: the route took all of q, answered as the oracle and as the scan, and flagged
    "few" = fewer than an eighth of the queries (a condition: a route that flags everything must not pass on the scan), "some" = not
    all of them, "all" = every one"""
    nq = q.shape[0]
    (d, i), stat, (sd, si) = _search_both(idx, q, k)
    print(what, "k", k, "per", per, "layout", _layout(min(per, nq)), "last", _layout(nq - (nq - 1) // per * per), "route (queries, flagged)", stat)
    assert stat[0] == nq, (what, "the search did not take the route", stat)
    bad = _same(d, i, od[:nq], oi[:nq], skip)
    assert not bad, (what, "k", k, "against the oracle: (query, piece, index in the piece)", _where(bad, per), "of", len(bad))
    bad = _same(d, i, sd, si, skip)
    assert not bad, (what, "k", k, "against scan_mfma 0: (query, piece, index in the piece)", _where(bad, per), "of", len(bad))
    if flagged == "few":
        assert 8 * stat[1] < nq, (what, "flagged queries", stat)
    elif flagged == "some":
        assert stat[1] < nq, (what, "flagged queries", stat)
    elif flagged == "all":
        assert stat == (nq, nq), (what, "flagged queries", stat)
    return d, i, stat


# A. three chunks and more in one piece: spx 8, mf_theta_kernel<16>.  513 queries = 3 chunks of 192, the last one holds 129 queries: four
# whole query blocks and query 512 alone in a fifth; 600 = 3 x 224, the last chunk 152 queries; 1100 = 5 x 224, the last chunk 204
@pytest.mark.parametrize("nq,k", [(513, 100), (600, 100), (600, 10), (1100, 100)])
def test_three_chunks_and_more_in_one_piece(amd, orc, world, nq, k):
    assert nq > 512 and _plan(D, SMALL, nq, k) == (nq, 1) and _layout(nq)[0] >= 3 and _layout(nq)[2] == 8
    idx = _index(amd, world, world.codes[:SMALL])
    try:
        od, oi = _oracle(orc, world, SMALL, k)
        d, i, _ = _check(idx, world.q[:nq], k, od, oi, "8229 rows x %d queries" % nq, nq)
        if nq == 513:
            assert np.array_equal(i[512], oi[512]) and np.array_equal(bits(d[512]), bits(od[512])), "query 512: the only one of the last chunk's fifth block"
    finally:
        idx.close()


# B. more than one piece: (rows, queries, k) -> (queries per piece, pieces), as pinned in test_adc_mfma_plan.py.  First / last piece:
#   1536: 3 x 256 twice          1537: 4 x 256, then 513 = 3 x 192         1700: 4 x 256, then 676 = 3 x 256
#   2100: 5 x 256, then 820 = 4 x 224                                       2500: 3 x 256 three times, then 196 = 1 chunk of 224, spx 32
#   3100: 4 x 256 three times, then 28 = 1 chunk of 32, spx 32, 4096 sample slots per query where the pieces before had 1024
#   20000 rows x 3100: 7 x 256, then 1308 = 6 x 224                         97 rows x 300: one chunk, then 44 = one chunk of 64
PIECES = [
    (SMALL, 1536, 100, 768, 2), (SMALL, 1537, 100, 1024, 2), (SMALL, 1700, 100, 1024, 2), (SMALL, 1700, 128, 1024, 2),
    (SMALL, 2100, 10, 1280, 2), (SMALL, 2100, 1, 1280, 2), (SMALL, 2500, 128, 768, 4), (SMALL, 3100, 100, 1024, 4),
    (ROWS, 3100, 100, 1792, 2), (TINY, 300, 1, 256, 2),
]


@pytest.mark.parametrize("n,nq,k,per,pieces", PIECES)
def test_pieces(amd, orc, world, n, nq, k, per, pieces):
    assert pieces > 1 and _plan(D, n, nq, k) == (per, pieces) and (pieces - 1) * per < nq <= pieces * per
    idx = _index(amd, world, world.codes[:n])
    try:
        od, oi = _oracle(orc, world, n, k)
        # (97 rows: the sample's four slots hold a row each, 1.25 k at k = 1 -- nothing the case relies on keeps the flagged count small)
        _check(idx, world.q[:nq], k, od, oi, "%d rows x %d queries" % (n, nq), per, flagged="some" if n == TINY else "few")
    finally:
        idx.close()


# D. flags raised in the first piece, at the first query of the second one and at the last query of the call; the launches per piece and per call
def test_nan_queries_in_two_pieces(amd, orc, world):
    import torch
    nq, k, per = 1700, 100, 1024
    assert _plan(D, SMALL, nq, k) == (per, 2)
    nan = (5, per, nq - 1)
    q = world.q[:nq].copy()
    for f in nan:
        q[f, 3] = np.nan
    idx = _index(amd, world, world.codes[:SMALL])
    try:
        od, oi = _oracle(orc, world, SMALL, k)
        idx.search(torch.from_numpy(np.ascontiguousarray(world.q[:nq])).cuda(), k)
        f0 = idx.last_mfma()[1]
        _, _, stat = _check(idx, q, k, od, oi, "NaN queries 5, 1024, 1699", per, flagged=None, skip=nan)
        print("flagged without the NaNs", f0, "with them", stat[1])
        assert 3 <= stat[1] <= f0 + 3, (f0, stat)
        with amd.launch_log() as log:
            idx.search(torch.from_numpy(q).cuda(), k)
        torch.cuda.synchronize()
        names = [rec[0] for rec in log]
        assert names.count("mf_select_kernel") == 2 and names.count("mf_theta_kernel") == 2, names
        for name in ("mf_compact_kernel", "mf_redo_bound_kernel", "mf_redo_tau_kernel", "mf_redo_collect_kernel", "mf_redo_finish_kernel"):
            assert names.count(name) == 1, (name, names)
    finally:
        idx.close()


# E. a list cap of 2 flags every query: 64 of them take the redo's slots (slot_q: queries of the first piece), all the others go through
# rest[q] with q in later pieces
@pytest.mark.parametrize("n,nq,k,per,pieces", [(SMALL, 1700, 100, 1024, 2), (SMALL, 3100, 10, 1792, 2), (TINY, 300, 100, 256, 2)])
def test_every_query_flagged_across_pieces(amd, orc, world, n, nq, k, per, pieces):
    assert pieces > 1 and _plan(D, n, nq, k, cap=2) == (per, pieces)
    idx = _index(amd, world, world.codes[:n], scan_mfma_cap=2)
    try:
        od, oi = _oracle(orc, world, n, k)
        d, i, _ = _check(idx, world.q[:nq], k, od, oi, "cap 2, %d rows x %d queries" % (n, nq), per, flagged="all")
        if k > n:
            assert np.all(i[:, n:] == -1) and np.all(np.isposinf(d[:, n:])) and np.all(i[:, :n] >= 0)
    finally:
        idx.close()


# F. id_base, and searches of other layouts in between on one handle: the scratch is kept, 1700 (4 x 256 + 3 x 256), 513 (3 x 192), 1700 again
def test_id_base_and_a_second_search_on_the_handle(amd, orc, world):
    nq, k, per = 1700, 100, 1024
    assert _plan(D, SMALL, nq, k) == (per, 2) and _plan(D, SMALL, 513, k) == (513, 1)
    idx = _index(amd, world, world.codes[:SMALL])
    try:
        idx.set_id_base(BASE)
        od, oi = _oracle(orc, world, SMALL, k)
        d1, i1, _ = _check(idx, world.q[:nq], k, od, oi + BASE, "id_base, 1700 queries", per)
        _check(idx, world.q[:513], k, od, oi + BASE, "id_base, 513 queries behind them", 513)
        d3, i3, _ = _check(idx, world.q[:nq], k, od, oi + BASE, "id_base, 1700 queries again", per)
        assert np.array_equal(i1, i3) and np.array_equal(bits(d1), bits(d3))
        assert i1.min() >= BASE
    finally:
        idx.close()


# G. other widths on this caller: D = 32 (one K step, codewords of 2), 96 (three K steps, four row tiles, the wide-row loop, codewords of
# 6), 256 (eight K steps, three row tiles, the wide-row loop; a permutation model); one chunk, three chunks, and at D = 96 two pieces
@pytest.mark.parametrize("d,nq,per,pieces", [(32, 40, 40, 1), (32, 600, 600, 1), (96, 40, 40, 1), (96, 600, 600, 1), (96, 1700, 1024, 2),
                                             (256, 40, 40, 1), (256, 600, 600, 1)])
def test_widths(amd, orc, d, nq, per, pieces):
    k = 50
    assert _plan(d, SMALL, nq, k) == (per, pieces)
    w = _width_world(amd, orc, d)
    idx = _index(amd, w, w.codes)
    try:
        od, oi = _oracle(orc, w, SMALL, k)
        _check(idx, w.q[:nq], k, od, oi, "D = %d, 8229 rows x %d queries" % (d, nq), per)
    finally:
        idx.close()


# H. a record region that runs over: 262 149 rows (the 20 000 thirteen times over and a ragged tail) x 4096 queries, one piece of
# 16 chunks x 256, regions of 1418 records.  The queries of a chunk whose region ran over are flagged as a whole (pass_flag).
# Measured on an MI355X, this shape at the default sample of one group in two: (4096, 4096) -- a region of every one of the 16 chunks runs
# over; so at 3072 queries (regions of 1953 records).  At 2048 queries (8 chunks, regions of 3046) none does and 632 queries raise their
# own flags (by elimination their lists, over 4096 rows: every row is there thirteen times); 302 of 1024, 149 of 513, 10 of 256.  With scan_mfma_sample 1 the
# regions hold at 4096 queries and 237 are flagged; at k = 10 nothing is flagged at any of these sizes.
def test_a_record_region_runs_over(amd, orc, world):
    import torch
    n, nq, k = 262149, 4096, 100
    assert _plan(D, n, nq, k) == (nq, 1) and _layout(nq) == (16, 256, 8) and _plan(D, n, nq // 2, k) == (nq // 2, 1)
    codes = np.concatenate([np.tile(world.codes, (13, 1)), world.codes[:2149]])[:n]
    extra = world.q[:nq - NQ].copy()
    extra[:, 1] += np.float32(1e-3)
    q = np.concatenate([world.q, extra])
    assert len(np.unique(q, axis=0)) == nq
    pick = [c * 256 + o for c in range(16) for o in (0, 31, 128, 255)]
    idx = _index(amd, world, codes)
    try:
        od, oi = orc.adc_search(orc.rotate_fma(world.rot["R"], q[pick]), world.books, codes, k)
        (d, i), stat, (sd, si) = _search_both(idx, q, k)
        print("262149 rows x 4096 queries: route (queries, flagged)", stat)
        assert stat[0] == nq, stat
        bad = _same(d, i, sd, si)
        assert not bad, ("against scan_mfma 0: (query, chunk, index in the chunk)", _where(bad, 256), "of", len(bad))
        bad = _same(d[pick], i[pick], od, oi)
        assert not bad, ("against the oracle", [pick[f] for f in bad])
        assert stat[1] >= 256, ("no record region ran over", stat)
        # The first half of the batch alone: half the chunks, so regions of twice the records.  Thresholds, margins and lists are a query's
        # own, so whoever is flagged now would be flagged in the full batch too; that NOT all of them are says the full batch's flags came
        # from its layout -- the regions.  The flagged ones outnumber the redo's slots: flagged and unflagged queries side by side, rest[q].
        d2, i2 = (t.cpu().numpy() for t in idx.search(torch.from_numpy(q[:nq // 2]).cuda(), k))
        half = idx.last_mfma()
        print("262149 rows x 2048 queries: route (queries, flagged)", half)
        assert half[0] == nq // 2 and half[1] < nq // 2, half
        bad = _same(d2, i2, sd[:nq // 2], si[:nq // 2])
        assert not bad, ("2048 queries against scan_mfma 0: (query, chunk, index in the chunk)", _where(bad, 256), "of", len(bad))
    finally:
        idx.close()
