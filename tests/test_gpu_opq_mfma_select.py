"""The selection behind the int8 matrix-core bound filter (mf_select_kernel, cvt_amd/csrc/adc_mfma.hip) against the oracle: ids with
np.array_equal, distances by bit pattern.

One wave per query reads the query's list, finds the k-th largest score, gives the rows inside the band below it their exact sums, keeps
everything at or below the k-th smallest sum (up to MF_KEEP = 512 rows) and sorts it by (distance, row).  What can go wrong there depends
on the list: its length against the 64 lanes of the wave and against the 1024 entries of the short form, the size of the band (several
rounds of 64 rows), ties across the k-th place, more ties than the selection keeps, k = 1, k = 128, k beyond the number of rows.  The
shapes below are the smallest that reach each of those."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

D, M, K = 128, 16, 256
SMALL = 8192 + 37
LARGE = 65536 + 37
NQ = 300


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()
    return cvt_amd


@pytest.fixture(scope="module")
def world(amd, orc):
    """codebooks trained on SIFT-like rows, 65 573 encoded rows, 300 queries; shared by the cases, never written"""
    from cvt_amd import synth
    w = type("World", (), {})()
    w.R = synth.random_rotation(D, seed=11)
    x = synth.sift_like(LARGE, D, seed=0xC0DE, device="cuda")
    probe = amd.OpqIndex(np.zeros((1, D), np.float32), np.zeros((M, K, D // M), np.float32), R=w.R)
    w.books = synth.train_books(probe.rotate(x[:8192]), M, K, iters=2).astype(np.float32)
    probe.close()
    enc = amd.OpqIndex(np.zeros((1, D), np.float32), w.books, R=w.R)
    _, codes = enc.rotate_encode(x)
    enc.close()
    w.codes = codes.cpu().numpy()
    w.q = synth.sift_like(NQ, D, seed=0xBEEF, device="cuda").cpu().numpy()
    w.q_rot = orc.rotate_fma(w.R, w.q)
    w.memo = {}
    return w


def _oracle(orc, w, tag, nq, codes, k):
    key = (tag, nq, k)
    if key not in w.memo:
        w.memo[key] = orc.adc_search(w.q_rot[:nq], w.books, codes, k)
    return w.memo[key]


def _route(amd, w, codes, q, k, od, oi, what, rows=None, log=False):
    """one search over `codes` on the route against (od, oi); -> ((queries, flagged) of the route, the kernels that ran)"""
    import torch
    idx = amd.OpqIndex(np.zeros((1, D), np.float32), w.books, R=w.R)
    ran = []
    try:
        idx.add_codes(codes)
        for name, v in (("scan_mfma_min_nq", 1), ("scan_mfma_min_rows", 1), ("profile", 1)):
            idx.set_param(name, v)
        qd = torch.from_numpy(np.ascontiguousarray(q)).cuda()
        if log:
            with amd.launch_log() as entries:
                d, i = idx.search(qd, k)
            ran = [e[0] for e in entries]
        else:
            d, i = idx.search(qd, k)
        stat = idx.last_mfma()
        d, i = d.cpu().numpy(), i.cpu().numpy()
    finally:
        idx.close()
    print(what, "k", k, "route (queries, flagged)", stat)
    assert stat[0] == q.shape[0], (what, "the search did not take the route", stat)
    rows = range(q.shape[0]) if rows is None else rows
    bad = [f for f in rows if not (np.array_equal(i[f], oi[f]) and np.array_equal(bits(d[f]), bits(od[f])))]
    assert not bad, (what, "k", k, "against the oracle", bad[:8])
    return stat, ran


def _with_copies(orc, w, n, rank, copies):
    """the first n rows and `copies` more of query 0's row of that rank (0 = best), appended -> (codes, that row)"""
    key = ("rank", n, rank)
    if key not in w.memo:
        w.memo[key] = int(orc.adc_search(w.q_rot[:1], w.books, w.codes[:n], rank + 1)[1][0, rank])
    row = w.memo[key]
    return np.concatenate([w.codes[:n], np.repeat(w.codes[row:row + 1], copies, axis=0)]), row


# 300 queries over 8229 rows: on so small an index a large share of the rows passes the threshold, the bands hold hundreds of rows --
# several rounds of 64 for the wave -- and the 300 lists differ in length
@pytest.mark.parametrize("k", [1, 100, 128])
def test_bands_of_hundreds_of_rows(amd, orc, world, k):
    od, oi = _oracle(orc, world, "small", NQ, world.codes[:SMALL], k)
    stat, _ = _route(amd, world, world.codes[:SMALL], world.q, k, od, oi, "8229 rows x 300 queries")
    assert stat[1] < NQ, ("every query went to the exact scan: the selection decided nothing", stat)


def test_k_beyond_the_rows(amd, orc, world):
    """31 rows, k = 100: every row is in the answer, the places behind them hold (+inf, -1)"""
    od, oi = _oracle(orc, world, "n31", 33, world.codes[:31], 100)
    assert (oi[:, 31:] == -1).all() and (oi[:, :31] >= 0).all()
    _route(amd, world, world.codes[:31], world.q[:33], 100, od, oi, "31 rows x 33 queries")


def test_ties_across_the_kth_place(amd, orc, world):
    """400 copies of query 0's 50th row: 401 rows share the distance the 100th place falls on, the selection keeps 450 rows (under MF_KEEP)
    and the lowest ids among the equals win"""
    codes, row = _with_copies(orc, world, SMALL, 49, 400)
    od, oi = _oracle(orc, world, "ties400", 33, codes, 100)
    assert oi[0, 49] == row and (oi[0, 50:] == np.arange(SMALL, SMALL + 50)).all(), oi[0, 45:55]
    stat, _ = _route(amd, world, codes, world.q[:33], 100, od, oi, "400 copies of the 50th row")
    assert stat[1] < 33, stat


def test_more_ties_than_the_selection_keeps(amd, orc, world):
    """600 copies: more rows at the k-th distance than MF_KEEP -- query 0 is flagged and the exact scan answers it"""
    codes, row = _with_copies(orc, world, SMALL, 49, 600)
    od, oi = _oracle(orc, world, "ties600", 33, codes, 100)
    assert oi[0, 49] == row
    stat, _ = _route(amd, world, codes, world.q[:33], 100, od, oi, "600 copies of the 50th row")
    assert stat[1] >= 1, ("query 0 has 601 rows at its 100th distance: the selection cannot have answered it", stat)


@pytest.fixture(scope="module")
def long_list(amd, orc, world):
    """65 573 rows and 1100 copies of query 0's 150th row behind them: the copies pass query 0's threshold with the row they repeat (they
    are no nearer than the 100th row, so the answer does not hold them), and its list is longer than the 1024 entries of the short form"""
    codes, _ = _with_copies(orc, world, LARGE, 149, 1100)
    od, oi = _oracle(orc, world, "long", 33, codes, 100)
    assert (oi[0] < LARGE).all()
    stat, ran = _route(amd, world, codes, world.q[:33], 100, od, oi, "1100 copies of the 150th row", log=True)
    bd, bi = _oracle(orc, world, "large", 33, world.codes[:LARGE], 100)
    base, _ = _route(amd, world, world.codes[:LARGE], world.q[:33], 100, bd, bi, "the same rows without the copies")
    return stat, ran, base


def test_list_longer_than_the_short_form(long_list):
    """the selection itself answers query 0 and its long list: the copies flag no query that the same rows without them do not flag (a
    long form that gave its queries to the exact scan would pass the comparison with the oracle all the same)"""
    stat, ran, base = long_list
    assert "mf_select_kernel" in ran, ran
    assert stat[1] <= base[1] < 33, ("flagged with the copies, without them", stat, base)


def test_long_lists_take_a_launch_of_their_own(long_list):
    """lists of more than 1024 entries are selected by mf_select_long_kernel (the same body over 4096 slots), launched behind the short form"""
    _, ran, _ = long_list
    assert "mf_select_long_kernel" in ran, ran
    assert ran.index("mf_select_long_kernel") > ran.index("mf_select_kernel"), ran


def test_nan_query_inside_the_batch(amd, orc, world):
    q = world.q[:64].copy()
    q[5, 3] = np.nan
    od, oi = _oracle(orc, world, "small", NQ, world.codes[:SMALL], 100)
    stat, _ = _route(amd, world, world.codes[:SMALL], q, 100, od[:64], oi[:64], "NaN query", rows=[f for f in range(64) if f != 5])
    assert 1 <= stat[1] < 64, stat
