"""The exact redo of the flagged queries on the "scan_mfma" route (mf_redo_* in cvt_amd/csrc/adc_mfma.hip): up to 64 flagged queries take a
slot and are answered over all rows by bound, collect and finish; the others, and a slot that cannot answer, go through the scan under
rest[q].  A list cap of 2 ("scan_mfma_cap") flags every query whose list holds more than two rows or fewer than k: with k > 2 that is
every query.  Against the oracle: ids with np.array_equal, distances by bit pattern; cvtmi_opq_last_mfma gives the flagged count, the
launch log tells which kernels answered."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

D, M, K = 128, 16, 256
ROWS, NQ, SMALL = 20000, 100, 8192 + 37
REDO = ("mf_compact_kernel", "mf_redo_bound_kernel", "mf_redo_tau_kernel", "mf_redo_collect_kernel", "mf_redo_finish_kernel")
GONE = ("adc_scan_kernel", "mf_scatter_kernel", "mf_count_kernel")


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()
    return cvt_amd


@pytest.fixture(scope="module")
def world(amd, orc):
    """codebooks trained on SIFT-like rows, 20 000 encoded rows, 100 queries and the oracle's answers; shared by the cases, never written"""
    from cvt_amd import synth
    w = type("World", (), {})()
    w.R = synth.random_rotation(D, seed=11)
    x = synth.sift_like(ROWS, D, seed=0xC0DE, device="cuda")
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


def _oracle(orc, w, tag, codes, k, id_base=0):
    if (tag, k) not in w.memo:
        w.memo[(tag, k)] = orc.adc_search(w.q_rot, w.books, codes, k, id_base=id_base)
    return w.memo[(tag, k)]


def _run(amd, w, codes, nq, k, od, oi, what, flagged, id_base=0):
    """one search of the first nq queries with every query flagged: the answer against the oracle's, the flagged count, the launches"""
    import torch
    idx = amd.OpqIndex(np.zeros((1, D), np.float32), w.books, R=w.R)
    try:
        idx.add_codes(codes)
        for name, v in (("scan_mfma_min_nq", 1), ("scan_mfma_min_rows", 1), ("scan_mfma_cap", 2), ("profile", 1)):
            idx.set_param(name, v)
        if id_base:
            idx.set_id_base(id_base)
        qd = torch.from_numpy(np.ascontiguousarray(w.q[:nq])).cuda()
        with amd.launch_log() as log:
            d, i = idx.search(qd, k)
        torch.cuda.synchronize()
        stat = idx.last_mfma()
    finally:
        idx.close()
    names = [rec[0] for rec in log]
    print(what, "k", k, "route (queries, flagged)", stat, "launches", names)
    assert stat == (nq, flagged), (what, "queries and flagged queries", stat)
    d, i = d.cpu().numpy(), i.cpu().numpy()
    bad = [f for f in range(nq) if not (np.array_equal(i[f], oi[f]) and np.array_equal(bits(d[f]), bits(od[f])))]
    assert not bad, (what, "k", k, "against the oracle", bad[:8])
    for name in REDO:
        assert names.count(name) == 1, (what, name, names)
    # (a batch of four queries or more has the 8-query scan planned behind the route: the row-per-lane kernel has no part left)
    for name in GONE:
        assert name not in names, (what, name, names)
    return d, i


@pytest.mark.parametrize("k", [100, 128])
def test_every_query_through_the_redo(amd, orc, world, k):
    od, oi = _oracle(orc, world, "small", world.codes[:SMALL], k)
    _run(amd, world, world.codes[:SMALL], 48, k, od, oi, "8229 rows x 48 queries", 48)


def test_k_one(amd, orc, world):
    """every row three times, so that a list of the filter holds three rows at least and the cap of 2 flags every query at k = 1 too"""
    codes = np.repeat(world.codes[:SMALL // 3], 3, axis=0)
    assert codes.shape[0] == SMALL
    od, oi = _oracle(orc, world, "thrice", codes, 1)
    _run(amd, world, codes, 48, 1, od, oi, "8229 rows (each three times) x 48 queries", 48)


def test_fewer_rows_than_k(amd, orc, world):
    od, oi = _oracle(orc, world, "tiny", world.codes[:31], 100)
    d, i = _run(amd, world, world.codes[:31], 48, 100, od, oi, "31 rows", 48)
    assert np.all(i[:, 31:] == -1) and np.all(np.isposinf(d[:, 31:])) and np.all(i[:, :31] >= 0)


def test_large_index_with_id_base(amd, orc, world):
    """262 149 rows: 256 row slices of 1025 rows, the last one short"""
    codes = np.concatenate([np.tile(world.codes, (13, 1)), world.codes[:2149]])[:262149]
    base = 5_000_000_000
    od, oi = _oracle(orc, world, "large", codes, 10, id_base=base)
    _, i = _run(amd, world, codes, 48, 10, od, oi, "262149 rows, id_base", 48, id_base=base)
    assert i.min() >= base


@pytest.mark.parametrize("nq", [64, 65, 100])
def test_slots_run_out(amd, orc, world, nq):
    """64 flagged queries fill the slots; the 65th and later ones are answered through rest"""
    od, oi = _oracle(orc, world, "small", world.codes[:SMALL], 100)
    _run(amd, world, world.codes[:SMALL], nq, 100, od, oi, "%d flagged queries" % nq, nq)


@pytest.mark.parametrize("copies", [400, 1100])
def test_copies_of_the_50th_row(amd, orc, world, copies):
    """Query 0's 50th row `copies` times over, away from its hundred best rows: 400 rows tie across the k-th place and the lower ids
    win; 1100 are more than the slot's list of 1024 holds, and the query goes through rest."""
    _, oi = _oracle(orc, world, "small", world.codes[:SMALL], 100)
    free = np.setdiff1d(np.arange(SMALL), oi[0])
    at = np.random.default_rng(copies).choice(free, copies, replace=False)
    codes = world.codes[:SMALL].copy()
    codes[at] = codes[oi[0, 49]]
    od, oi2 = _oracle(orc, world, "copies %d" % copies, codes, 100)
    assert np.all(bits(od[0, 49:]) == bits(od[0, 49])) and np.all(np.diff(oi2[0, 49:]) > 0)   # the case is what it says
    _run(amd, world, codes, 48, 100, od, oi2, "%d copies" % copies, 48)
