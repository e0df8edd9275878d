"""The int8 row-tile filter kernel (flat_u8_tfilter_kernel, cvt_amd/csrc/flat_u8_tfilter.hip) at the group boundaries of a wave's loop,
through both of its callers.

A wave of the kernel walks tile groups of RT row tiles (RT = 3 at 128-d: 96 rows; RT = 4 below) with a stride of one group per wave
stream, so what can go wrong at a boundary -- a group fetched ahead that does not exist, the clamp of the last ragged tile, the start
values of rows past the end, the sample's mapping of its groups onto all groups -- depends on how many groups a wave gets, not on the
table's size.  The row counts below are chosen by wave streams: no group for most waves, exactly one for every wave, two for a single
wave, a tile count that is no multiple of RT.

ADC route ("scan_mfma", adc_mfma.hip; 8 spx x 8 streams per query chunk): the oracle's adc_search is the truth, ids with array_equal,
distances by bit pattern, and cvtmi_opq_last_mfma tells that the search took the route.  Flat uint8 caller (UT_GRID x UT_WAVES = 2048
streams for one chunk of queries): against the exact uint8 kernels ("flat_u8_tfilter" 0) on every query."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

D, M, K = 128, 16, 256
GROUP = 96                       # rows of a tile group at 128-d (RT = 3)
ONE_CHUNK = 8 * 32 * 8           # wave streams of a batch of up to 256 queries (chunks = 1, spx = 32)
TWO_CHUNKS = 8 * 16 * 8          # ... and per chunk of 257 .. 512 queries (chunks = 2, spx = 16)
ROWS = ONE_CHUNK * GROUP + GROUP + 5
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
    """codebooks trained on SIFT-like rows, 196 709 encoded rows, 300 queries; shared by the cases, never written"""
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


def _oracle(orc, w, n, nq, k):
    """the oracle's answer over the first n rows for the first nq queries, computed once per shape"""
    key = (n, nq, k)
    if key not in w.memo:
        w.memo[key] = orc.adc_search(w.q_rot[:nq], w.books, w.codes[:n], k)
    return w.memo[key]


def _route(amd, w, codes, q, k, od, oi, what, sample=None):
    """one search over `codes` on the route against (od, oi); -> (queries, flagged) of the route"""
    import torch
    idx = amd.OpqIndex(np.zeros((1, D), np.float32), w.books, R=w.R)
    try:
        idx.add_codes(codes)
        for name, v in (("scan_mfma_min_nq", 1), ("scan_mfma_min_rows", 1), ("profile", 1)):
            idx.set_param(name, v)
        if sample is not None:
            idx.set_param("scan_mfma_sample", sample)
        d, i = idx.search(torch.from_numpy(np.ascontiguousarray(q)).cuda(), k)
        stat = idx.last_mfma()
        d, i = d.cpu().numpy(), i.cpu().numpy()
    finally:
        idx.close()
    print(what, "k", k, "route (queries, flagged)", stat)
    assert stat[0] == q.shape[0], (what, "the search did not take the route", stat)
    bad = [f for f in range(q.shape[0]) if not (np.array_equal(i[f], oi[f]) and np.array_equal(bits(d[f]), bits(od[f])))]
    assert not bad, (what, "k", k, "against the oracle", bad[:8])
    return stat


# fewer rows than a group (most waves get none: nothing may be fetched ahead for them), the group itself, one row more
@pytest.mark.parametrize("k", [100, 10])
@pytest.mark.parametrize("n", [1, 31, 95, 96, 97])
def test_adc_at_most_two_groups(amd, orc, world, n, k):
    od, oi = _oracle(orc, world, n, 33, k)
    _route(amd, world, world.codes[:n], world.q[:33], k, od, oi, "%d rows x 33 queries" % n)


# one chunk of queries, 2048 streams: every wave exactly one group (a second must not be fetched); one wave two groups and a ragged last tile
@pytest.mark.parametrize("k", [100, 10])
@pytest.mark.parametrize("n", [ONE_CHUNK * GROUP, ROWS])
def test_adc_one_group_per_wave_and_one_more(amd, orc, world, n, k):
    od, oi = _oracle(orc, world, n, 64, k)
    stat = _route(amd, world, world.codes[:n], world.q[:64], k, od, oi, "%d rows x 64 queries" % n)
    assert stat[1] < 64, ("every query went to the exact scan: the filter decided nothing", stat)


# two chunks of queries, 1024 streams each
@pytest.mark.parametrize("k", [100, 10])
def test_adc_two_chunks_one_wave_with_two_groups(amd, orc, world, k):
    n = TWO_CHUNKS * GROUP + GROUP + 5
    od, oi = _oracle(orc, world, n, NQ, k)
    stat = _route(amd, world, world.codes[:n], world.q, k, od, oi, "%d rows x 300 queries" % n)
    assert stat[1] < NQ, ("every query went to the exact scan: the filter decided nothing", stat)


# a tile count that is no multiple of RT: the last group's missing tiles are clamped, and the ragged last tile holds a row of the answer
@pytest.mark.parametrize("k", [100, 10])
@pytest.mark.parametrize("tiles", [625, 626])
def test_adc_last_group_short_of_tiles(amd, orc, world, tiles, k):
    n = (tiles - 1) * 32 + 5
    assert tiles % 3 == tiles - 624
    key = ("planted", tiles, k)
    if key not in world.memo:
        best = orc.adc_search(world.q_rot[:1], world.books, world.codes[:n - 1], 1)[1][0, 0]
        codes = world.codes[:n].copy()
        codes[n - 1] = codes[best]                    # query 0's best row once more, as the last row of the ragged tile
        world.memo[key] = (codes, best) + tuple(orc.adc_search(world.q_rot[:33], world.books, codes, k))
    codes, best, od, oi = world.memo[key]
    assert oi[0, 0] == best and oi[0, 1] == n - 1, (oi[0, :3], best, n)
    _route(amd, world, codes, world.q[:33], k, od, oi, "%d tiles x 33 queries" % tiles)


# few rows, many queries: the 86 waves that get a group meet five query blocks each, and on so small an index a large share of the rows
# passes a query's threshold -- a wave writes hundreds of records into its region, from every block of a group and most of its tiles
@pytest.mark.parametrize("k", [100, 10])
def test_adc_many_records_per_wave(amd, orc, world, k):
    n = 8192 + 37
    od, oi = _oracle(orc, world, n, NQ, k)
    _route(amd, world, world.codes[:n], world.q, k, od, oi, "%d rows x 300 queries" % n)


# the sample's groups mapped onto all groups: every group (1) and one in three on the shape where one wave has two
@pytest.mark.parametrize("sample", [1, 3])
def test_adc_sample_divisor(amd, orc, world, sample):
    od, oi = _oracle(orc, world, ROWS, 64, 100)
    _route(amd, world, world.codes[:ROWS], world.q[:64], 100, od, oi, "sample %d" % sample, sample=sample)


# ---- the flat uint8 caller of the same kernel ----

L2U8 = 2
U8_STREAMS = 256 * 8             # UT_GRID x UT_WAVES: one chunk of queries


def _flat(amd, db, q, k, tfilter):
    amd.set_tuning("flat_u8_tfilter", tfilter)
    try:
        ix = amd.FlatIndex(L2U8, db.shape[1])
        try:
            ix.add(db)
            with amd.launch_log() as log:
                d, i = ix.search(q, k)
            last = ix.last_search()
        finally:
            ix.close()
    finally:
        amd.set_tuning("flat_u8_tfilter", 1)
    return np.asarray(d), np.asarray(i), [e[0] for e in log], last


@pytest.mark.parametrize("two_groups", [False, True])
@pytest.mark.parametrize("width", [32, 64, 96, 128])
def test_flat_u8_widths(amd, width, two_groups):
    """k = 129: every batch takes the filter.  65 573 rows leave most waves one group or none; the second count gives every wave a group
    and one wave two, with a ragged last tile"""
    rt = 3 if width >= 128 else 4
    n = U8_STREAMS * 32 * rt + 32 * rt + 5 if two_groups else 65536 + 37
    nq, k = 33, 129
    rng = np.random.default_rng(width + n)
    db = rng.integers(0, 256, size=(n, width), dtype=np.uint8)
    q = rng.integers(0, 256, size=(nq, width), dtype=np.uint8)
    db[n - 1] = db[2]; db[n // 2] = db[2]; q[0] = db[2]       # ties at the top, one of them the last row
    d, i, ran, last = _flat(amd, db, q, k, 1)
    assert ran.count("flat_u8_tfilter_kernel") == 2 and last[0] == 4, (ran, last)   # the sample pass and the filter pass
    xd, xi, xran, _ = _flat(amd, db, q, k, 0)
    assert "flat_u8_tfilter_kernel" not in xran, xran
    assert d.dtype == np.int32 and xd.dtype == np.int32
    bad = np.flatnonzero(np.any(i != xi, axis=1) | np.any(d != xd, axis=1))
    assert bad.size == 0, (width, n, "queries", bad[:8].tolist())
    assert i[0, 0] == 2 and i[0, 1] == n // 2 and i[0, 2] == n - 1, i[0, :4]
