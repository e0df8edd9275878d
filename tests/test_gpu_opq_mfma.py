"""The int8 matrix-core bound filter of large ADC batches (cvt_amd/csrc/adc_mfma.hip, "scan_mfma") against the oracle and against the scan
it stands in front of: ids with np.array_equal, distances by bit pattern.  The lower bounds of the route are set down through set_param so
that small shapes take it; cvtmi_opq_last_mfma tells whether a search took the route and how many of its queries the exact scan had to
answer, so a case cannot pass on the fall-back alone unless it is about the fall-back."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

D, M, K = 128, 16, 256
ROWS, NQ = 20000, 300


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()
    return cvt_amd


@pytest.fixture(scope="module")
def world(amd, orc):
    """codebooks trained on SIFT-like rows, 23 000 encoded rows, 300 queries; everything the cases share, never written"""
    from cvt_amd import synth
    w = type("World", (), {})()
    w.R = synth.random_rotation(D, seed=11)
    x = synth.sift_like(ROWS + 3000, D, seed=0xC0DE, device="cuda")
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


def _index(amd, w, codes, books=None, **kw):
    if "perm" not in kw:
        kw["R"] = w.R
    idx = amd.OpqIndex(np.zeros((1, D), np.float32), w.books if books is None else books, **kw)
    idx.add_codes(codes)
    for name, v in (("scan_mfma_min_nq", 1), ("scan_mfma_min_rows", 1), ("profile", 1)):
        idx.set_param(name, v)
    return idx


def _oracle(orc, w, tag, q_rot, codes, k, books=None, id_base=0):
    key = (tag, k)
    if key not in w.memo:
        w.memo[key] = orc.adc_search(q_rot, w.books if books is None else books, codes, k, id_base=id_base)
    return w.memo[key]


def _same(d, i, od, oi, rows=None):
    d, i = d.cpu().numpy(), i.cpu().numpy()
    rows = range(d.shape[0]) if rows is None else rows
    return [f for f in rows if not (np.array_equal(i[f], oi[f]) and np.array_equal(bits(d[f]), bits(od[f])))]


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
    return got, stat, ref


def _check(idx, q, k, od, oi, what, flagged=0, rows=None):
    (d, i), stat, (sd, si) = _search_both(idx, q, k)
    print(what, "k", k, "route (queries, flagged)", stat)
    assert stat[0] == q.shape[0], (what, "the search did not take the route", stat)
    bad = _same(d, i, od, oi, rows)
    assert not bad, (what, "k", k, "against the oracle", bad[:8])
    bad = _same(d, i, sd.cpu().numpy(), si.cpu().numpy(), rows)
    assert not bad, (what, "k", k, "against scan_mfma 0", bad[:8])
    if flagged is not None:
        assert stat[1] == flagged, (what, "flagged queries", stat)
    return stat


def test_ragged_tile_and_query_block(amd, orc, world):
    n = 8192 + 37
    idx = _index(amd, world, world.codes[:n])
    try:
        od, oi = _oracle(orc, world, "ragged", world.q_rot[:33], world.codes[:n], 100)
        _check(idx, world.q[:33], 100, od, oi, "8229 rows x 33 queries")
    finally:
        idx.close()


@pytest.mark.parametrize("k", [1, 100, 128])
def test_two_chunks_of_queries(amd, orc, world, k):
    idx = _index(amd, world, world.codes[:ROWS])
    try:
        od, oi = _oracle(orc, world, "base", world.q_rot, world.codes[:ROWS], k)
        _check(idx, world.q, k, od, oi, "20000 rows x 300 queries")
    finally:
        idx.close()


def test_equal_rows(amd, orc, world):
    """5000 copies of one row among other rows: a query next to them has 5000 rows at its best distance -- more than a list holds -- and goes
    to the exact scan; so may any query whose threshold the copies pass.  The answers are the oracle's either way."""
    codes = np.concatenate([np.repeat(world.codes[7:8], 5000, axis=0), world.codes[100:3100]])
    near = world.books[np.arange(M), world.codes[7]].reshape(1, D) + np.float32(0.5)      # next to the copies, in rotated space
    q_rot = np.concatenate([near, world.q_rot[:40]]).astype(np.float32)
    idx = _index(amd, world, codes)
    try:
        import torch
        od, oi = _oracle(orc, world, "equal", q_rot, codes, 100)
        d, i = idx.search(torch.from_numpy(q_rot).cuda(), 100, rotate=False)
        stat = idx.last_mfma()
        print("equal rows: route (queries, flagged)", stat)
        assert stat[0] == q_rot.shape[0] and stat[1] >= 1, stat
        assert not _same(d, i, od, oi)
    finally:
        idx.close()


def test_duplicate_rows_across_the_kth_place(amd, orc, world):
    """every row twice: an odd k cuts a pair of equal distances, the lower id stays"""
    codes = np.repeat(world.codes[:6000], 2, axis=0)
    idx = _index(amd, world, codes)
    try:
        od, oi = _oracle(orc, world, "twice", world.q_rot[:64], codes, 101)
        _check(idx, world.q[:64], 101, od, oi, "every row twice")
    finally:
        idx.close()


def test_nan_query_inside_a_batch(amd, orc, world):
    q = world.q[:64].copy()
    q[5, 3] = np.nan
    idx = _index(amd, world, world.codes[:ROWS])
    try:
        od, oi = _oracle(orc, world, "base", world.q_rot, world.codes[:ROWS], 100)
        _check(idx, q, 100, od[:64], oi[:64], "NaN query", flagged=1, rows=[f for f in range(64) if f != 5])
    finally:
        idx.close()


def test_list_cap_two_flags_every_query(amd, orc, world):
    idx = _index(amd, world, world.codes[:ROWS])
    try:
        idx.set_param("scan_mfma_cap", 2)
        od, oi = _oracle(orc, world, "base", world.q_rot, world.codes[:ROWS], 100)
        _check(idx, world.q[:48], 100, od[:48], oi[:48], "cap 2", flagged=48)
    finally:
        idx.close()


def test_more_flagged_queries_than_the_redo_batch_holds(amd, orc, world):
    """cap 2 with 100 queries: 64 go through the short redo batch, the others through the scan under the group predicate"""
    idx = _index(amd, world, world.codes[:ROWS])
    try:
        idx.set_param("scan_mfma_cap", 2)
        od, oi = _oracle(orc, world, "base", world.q_rot, world.codes[:ROWS], 100)
        _check(idx, world.q[:100], 100, od[:100], oi[:100], "cap 2, 100 queries", flagged=100)
    finally:
        idx.close()


def test_flagged_queries_of_a_large_index(amd, orc, world):
    """262 149 rows (the rows twelve times over and a ragged tail): the redo batch runs with its row splits and the predicated merge"""
    codes = np.concatenate([np.tile(world.codes[:ROWS], (13, 1)), world.codes[:2149]])[:262149]
    idx = _index(amd, world, codes)
    try:
        idx.set_param("scan_mfma_cap", 2)
        od, oi = _oracle(orc, world, "large", world.q_rot[:70], codes, 10)
        _check(idx, world.q[:70], 10, od, oi, "262149 rows, cap 2", flagged=70)
    finally:
        idx.close()


def test_another_width(amd, orc):
    """D = 64 (step 4, two K steps per row) with its own codebooks"""
    from cvt_amd import synth
    d = 64
    R = synth.random_rotation(d, seed=3)
    x = synth.sift_like(12000, d, seed=0xD64, device="cuda")
    probe = amd.OpqIndex(np.zeros((1, d), np.float32), np.zeros((M, K, d // M), np.float32), R=R)
    books = synth.train_books(probe.rotate(x[:8192]), M, K, iters=2).astype(np.float32)
    probe.close()
    idx = amd.OpqIndex(np.zeros((1, d), np.float32), books, R=R)
    try:
        _, codes = idx.rotate_encode(x)
        idx.add_codes(codes)
        for name, v in (("scan_mfma_min_nq", 1), ("scan_mfma_min_rows", 1), ("profile", 1)):
            idx.set_param(name, v)
        q = synth.sift_like(40, d, seed=0xBEEF, device="cuda").cpu().numpy()
        od, oi = orc.adc_search(orc.rotate_fma(R, q), books, codes.cpu().numpy(), 50)
        _check(idx, q, 50, od, oi, "D = 64")
    finally:
        idx.close()


def test_rows_appended_after_a_search(amd, orc, world):
    idx = _index(amd, world, world.codes[:ROWS])
    try:
        od, oi = _oracle(orc, world, "base", world.q_rot, world.codes[:ROWS], 100)
        _check(idx, world.q[:64], 100, od[:64], oi[:64], "before the append")
        idx.add_codes(world.codes[ROWS:])
        # (another batch size than before: the route's counters must be this search's, not the last one's)
        od, oi = _oracle(orc, world, "appended", world.q_rot[:48], world.codes, 100)
        _check(idx, world.q[:48], 100, od, oi, "after the append")
    finally:
        idx.close()


def test_rows_removed(amd, orc, world):
    idx = _index(amd, world, world.codes[:ROWS])
    try:
        od, oi = _oracle(orc, world, "base", world.q_rot, world.codes[:ROWS], 100)
        _check(idx, world.q[:64], 100, od[:64], oi[:64], "before the removal")
        gone = np.unique(np.concatenate([oi[:64, :3].ravel(), np.arange(31, ROWS, 97)])).astype(np.int64)   # best rows among them
        assert idx.remove_ids(gone) == gone.size
        keep = np.ones(ROWS, bool); keep[gone] = False
        od, oi = _oracle(orc, world, "removed", world.q_rot[:48], world.codes[:ROWS][keep], 100)
        _check(idx, world.q[:48], 100, od, oi, "after the removal")
    finally:
        idx.close()


def test_id_base(amd, orc, world):
    idx = _index(amd, world, world.codes[:ROWS])
    try:
        idx.set_id_base(5_000_000_000)
        od, oi = _oracle(orc, world, "base", world.q_rot, world.codes[:ROWS], 100)
        _check(idx, world.q[:64], 100, od[:64], oi[:64] + 5_000_000_000, "id_base")
    finally:
        idx.close()


def test_permutation_model(amd, orc, world):
    perm = np.random.default_rng(5).permutation(D).astype(np.int32)
    idx = _index(amd, world, world.codes[:ROWS], perm=perm)
    try:
        q_rot = idx.rotate(world.q[:64])
        od, oi = _oracle(orc, world, "perm", q_rot, world.codes[:ROWS], 100)
        _check(idx, world.q[:64], 100, od, oi, "permutation model")
    finally:
        idx.close()


def test_nonfinite_codebook_entry_stays_on_the_scan(amd, orc, world):
    books = world.books.copy()
    books[3, 200, 1] = np.inf
    codes = world.codes[:ROWS].copy()
    codes[codes[:, 3] == 200, 3] = 201            # no row reads the entry
    idx = _index(amd, world, codes, books=books)
    try:
        od, oi = _oracle(orc, world, "inf-book", world.q_rot[:64], codes, 100, books=books)
        (d, i), stat, _ = _search_both(idx, world.q[:64], 100)
        assert stat == (0, 0), stat
        assert not _same(d, i, od, oi)
    finally:
        idx.close()
