"""Every uint8 (L2U8) flat-search kernel family by name, at its tile, split and tie edges.

Six families answer a uint8 search: the dot4 row-per-lane kernels (flat_u8_kernel), the 32-query matrix-core kernel
(flat_u8_mfma_kernel), the row-tile kernels (flat_u8_rowtile_kernel), the stream with its selection (flat_u8_mstream_kernel +
flat_u8_stream_finish_kernel), the sample + filter pipeline (flat_variant 2) and the threshold filter (flat_u8_tfilter.hip, which keeps
its own tests: one route-pinning case here).  cvtmi_flat_last_search reports 0 for the first four alike, so every case here reads the
launch log (cvt_amd.launch_log) and asserts the kernel it was shaped for, its block and its split count where the log shows them, and
that no other uint8 search kernel ran.

The reference is a numpy model of the operation, not another kernel: |q|^2 + |x|^2 - 2 q.x over the first D // 4 * 4 dimensions (the
reference drops a D % 4 tail), the product as a float64 GEMM (every term is an integer below 2^53: exact), ordered by (distance, row),
padded with label -1 and the bits 0x7f800000.  Every query of every case is compared, distances and labels, exactly.  One CPU test
checks the model itself against the oracle."""
import contextlib

import numpy as np
import pytest

gpu = pytest.mark.gpu
L2U8 = 2
PAD = np.int32(0x7f800000)

# every kernel that computes or selects uint8 distances for a search (cvt_amd/csrc/flat.hip, flat_mfma.hip, flat_u8_tfilter.hip); the
# norms / operand-copy / merge / label kernels around them are not routes
DOT4, MFMA, ROWTILE = "flat_u8_kernel", "flat_u8_mfma_kernel", "flat_u8_rowtile_kernel"
STREAM = ("flat_u8_mstream_kernel", "flat_u8_stream_finish_kernel")
PIPE_FINISH = ("flat_scatter_kernel", "flat_u8_finish_kernel")
TFILTER = ("flat_u8_tfilter_kernel", "ut_theta_kernel", "ut_bucket_kernel", "ut_finish_kernel")
U8_SEARCH = {DOT4, MFMA, ROWTILE, *STREAM, *PIPE_FINISH, *TFILTER, "flat_u8_gfilter_kernel", "flat_u8_gfilter_wide_kernel", "flat_u8_filter_kernel"}

DEFAULTS = dict(flat_variant=0, flat_u8_tfilter=1, flat_u8_mstream_min=1, flat_u8_sample_passes=10, flat_u8_opt=0)
EXACT = dict(flat_variant=1)                                  # dot4 / mfma / row-tile by flat_u8_mfma_qtile
STREAMED = dict(flat_variant=0, flat_u8_tfilter=0)            # the stream wherever it applies
PIPELINE = dict(flat_variant=2)


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()
    return cvt_amd


# ---- the model ----

def model(db, q, k):
    """(distances int32 [nq][k], rows int64 [nq][k]) of the k nearest rows in (distance, row) order"""
    n, D = db.shape
    nq, D4 = q.shape[0], D // 4 * 4
    dist = np.empty((nq, k), np.int32); dist[:] = PAD
    rows = np.full((nq, k), -1, np.int64)
    kk = min(k, n)
    qf = q[:, :D4].astype(np.float64)
    qq = (qf * qf).sum(axis=1)
    step = max(2 * kk, min(n, (1 << 23) // max(nq, 1)))       # (blocks of rows: the key matrix of the largest case stays under 100 MB)
    best = np.empty((nq, 0), np.int64)
    for a in range(0, n, step):
        x = db[a:a + step, :D4].astype(np.float64)
        d = qq[:, None] + (x * x).sum(axis=1)[None, :] - 2.0 * (qf @ x.T)
        key = (d.astype(np.int64) << 32) | np.arange(a, a + len(x), dtype=np.int64)[None, :]      # distance < 2^29, row < 2^32
        key = np.concatenate([best, key], axis=1)             # one sortable word per (distance, row)
        best = np.partition(key, kk - 1, axis=1)[:, :kk] if kk < key.shape[1] else key
    best = np.sort(best, axis=1)
    dist[:, :kk] = (best >> 32).astype(np.int32)
    rows[:, :kk] = best & 0xffffffff
    return dist, rows


SMALL = [(1, 1, 1, 1), (7, 3, 2, 3), (40, 5, 3, 8), (300, 21, 5, 40), (129, 30, 4, 129), (64, 64, 9, 10), (1000, 128, 6, 100), (33, 520, 2, 5)]


@pytest.mark.parametrize("n,D,nq,k", SMALL)
def test_model_equals_the_oracle(orc, n, D, nq, k):
    """the numpy model against the CPU oracle's L2SqrI loop on small tables -- D = 3 (every distance 0: rows 0 .. k - 1) and D = 21 (a
    dropped tail) among them, duplicates, k above the row count -- so that the GPU cases below rest on a reference checked without a GPU"""
    rng = np.random.default_rng(n * 31 + D)
    db = rng.integers(0, 256 if D != 64 else 4, size=(n, D), dtype=np.uint8)
    q = rng.integers(0, 256 if D != 64 else 4, size=(nq, D), dtype=np.uint8)
    if n > 4:
        db[n - 1] = db[1]; db[n // 2] = db[1]; q[0] = db[1]
    _, odi, oi = orc.flat_search(L2U8, db, q, k)
    md, mi = model(db, q, k)
    assert np.array_equal(mi, oi) and np.array_equal(md, odi)
    if D < 4:
        assert np.array_equal(mi[:, :min(k, n)], np.tile(np.arange(min(k, n)), (nq, 1))) and np.all(md[:, :min(k, n)] == 0)
    if k > n:
        assert np.all(mi[:, n:] == -1) and np.all(md[:, n:].view(np.uint32) == 0x7f800000)


def test_model_equals_the_oracle_on_the_golden_tables(orc, golden):
    f = golden.flat
    for tag in ("u8a", "u8b", "u8c"):
        md, mi = model(f[tag + "_db"], f[tag + "_q"], 10)
        assert np.array_equal(md, f[tag + "_d"]) and np.array_equal(mi, f[tag + "_i"]), tag


# ---- host models of the planners (cvt_amd/csrc/flat.hip), to derive shapes and to read split counts off the grid ----

def plan_splits(n, nq, qt):                                   # flat_plan_splits
    groups = -(-nq // qt)
    return max(1, min(2048 // groups, max(n // 2048, 1), 1024))


def dot4_qt(nq, k):
    return 1 if k > 128 or nq < 4 else 4


def dot4_rows_per_split(n, splits):                           # launch_flat_search: whole 512-row tiles
    return max(512, -(-(-(-n // splits)) // 512) * 512)


def mfma_qtile(D, k, nq):                                     # flat_u8_mfma_qtile
    if D % 32 or D > 512 or nq < 5 or k > 128:
        return 0
    if k <= 24:
        return 256 if nq > 128 else (128 if nq > 64 else (64 if nq > 32 else 32))
    if k <= 80:
        return 128 if nq > 64 else 32
    return 32


def mfma_splits(n, nq, qt):                                   # flat_u8_mfma_splits + the XCD rounding of flat_search_rows
    if qt <= 32:
        s = plan_splits(n, nq, qt)
    else:
        s = max(1, min(-(-512 // -(-nq // qt)), max(n // 8192, 1)))
    return s // 8 * 8 if s >= 8 else s


def stream_slices(m):                                         # flat_u8_stream_finish_plan on tables this small
    s = 64
    while s > 8 and m * s > 1024:
        s //= 2
    return s


# ---- running a case ----

@contextlib.contextmanager
def tuned(amd, **keys):
    try:
        for name, value in keys.items():
            amd.set_tuning(name, value)
        yield
    finally:
        for name in keys:
            amd.set_tuning(name, DEFAULTS[name])


def search(amd, db, q, k, tune, seam=None):
    """the search under `tune` -> (distances, labels, {kernel name: [(grid, block, lds), ...]} of the uint8 search kernels, last_search())"""
    with tuned(amd, **tune):
        ix = amd.FlatIndex(L2U8, db.shape[1])
        try:
            if seam:
                ix.add(db[:seam]); ix.add(db[seam:])
            else:
                ix.add(db)
            with amd.launch_log() as log:
                d, i = ix.search(q, k)
            last = ix.last_search()
        finally:
            ix.close()
    ran = {}
    for name, grid, block, lds in log:
        if name in U8_SEARCH:
            ran.setdefault(name, []).append((grid, block, lds))
    return d, i, ran, last


def check(d, i, db, q, k, what):
    md, mi = model(db, q, k)
    bad = np.flatnonzero(np.any(i != mi, axis=1) | np.any(d != md, axis=1))
    assert d.dtype == np.int32 and bad.size == 0, (what, "queries", bad[:8].tolist(), i[bad[:1]].tolist(), mi[bad[:1]].tolist(), d[bad[:1]].tolist(), md[bad[:1]].tolist())


def table(seed, n, D, nq, hi=256):
    rng = np.random.default_rng(seed)
    db = rng.integers(0, hi, size=(n, D), dtype=np.uint8)
    q = rng.integers(0, hi, size=(nq, D), dtype=np.uint8)
    if n > 8:                                                 # (distance, row) ties at the top: a row three times, asked for by query 0
        db[n - 1] = db[2]; db[n // 2] = db[2]; q[0] = db[2]
    return db, q


def odd_seam(n):
    return (n // 2) | 1 if n > 2 else None                    # two appends whose seam is no multiple of 32 (nor of anything even)


# ---- the dot4 row-per-lane kernels: flat_u8_kernel<VEC, QT, CAP, TRIG> ----

DOT4_CASES = (
    # D: a byte, a dropped tail, the first word, 16-byte pieces (VEC) and not, past the matrix-core widths, the widest; D < 4: every distance 0
    [(513, D, 3, 5) for D in (1, 3, 5, 16, 21, 48, 520, 4096)] +
    # nq: QT 1 (nq < 4) and QT 4 with 0 .. 3 clamped padding queries
    [(1000, 21, nq, 10) for nq in (1, 3, 4, 5, 7)] +
    # k: the small and the large selection buffer, and a k above the row count
    [(3000, 48, 5, k) for k in (1, 128, 129, 2048)] + [(511, 16, 2, 2048), (3000, 21, 5, 129)] +
    # n: a row, one short of a 512-row tile, the tile, one past it (nq < 5: dot4 at a matrix-core width too)
    [(n, 32, 4, 10) for n in (1, 511, 512, 513)] +
    # split plans whose last split is empty / holds one row (derived in the test)
    [(12289, 128, 1, 10), (10241, 128, 1, 10), (12289, 21, 7, 10), (10241, 16, 4, 129)])


@gpu
@pytest.mark.parametrize("n,D,nq,k", DOT4_CASES)
def test_dot4_kernels(amd, n, D, nq, k):
    assert mfma_qtile(D, k, nq) == 0
    db, q = table(n * 7 + D + nq + k, n, D, nq)
    d, i, ran, last = search(amd, db, q, k, EXACT, seam=odd_seam(n))
    qt = dot4_qt(nq, k)
    splits = plan_splits(n, nq, qt)
    assert set(ran) == {DOT4} and last[0] == 0, ran
    assert ran[DOT4] == [((-(-nq // qt) * splits, 1, 1), 256, qt * (D // 4 + 1) * 4)], (ran, splits)
    if n in (12289, 10241):   # n // 2048 splits of whole 512-row tiles: 6 x 2560 -- the sixth starts at 12 800, past the table; 5 x 2560 -- the fifth holds row 10 240 alone
        rps = dot4_rows_per_split(n, splits)
        assert splits == n // 2048 and n - (splits - 1) * rps == (1 if n == 10241 else -511)
    check(d, i, db, q, k, (n, D, nq, k))


# ---- the 32-query matrix-core kernel: flat_u8_mfma_kernel<1, 208, 176, DMAX> ----

MFMA_CASES = [  # (n, D, nq, k): D across DMAX 128 / 512, n around the 32-row tile and the 128-row split unit, nq around the 32-query tile, k on each side of the rule
    (1, 32, 5, 1), (31, 96, 32, 81), (32, 128, 33, 128), (33, 160, 5, 1), (127, 512, 32, 81), (128, 128, 33, 128), (129, 160, 5, 128),
    (129, 512, 33, 81), (128, 96, 32, 1), (2000, 32, 32, 24), (300, 128, 64, 25), (300, 512, 32, 80),
    (10241, 128, 5, 10),       # 5 row splits: no multiple of 8
    (16384 + 77, 128, 33, 81),  # 8 row splits, one per XCD; two query groups
    (16384 + 77, 256, 5, 1)]


@gpu
@pytest.mark.parametrize("n,D,nq,k", MFMA_CASES)
def test_mfma_kernel(amd, n, D, nq, k):
    assert mfma_qtile(D, k, nq) == 32
    db, q = table(n * 5 + D + nq + k, n, D, nq)
    if n > 16384:             # the best row of query 1 again in a middle and in the last split: rows decide across splits
        db[9000] = db[11]; db[16400] = db[11]; q[1] = db[11]
    d, i, ran, last = search(amd, db, q, k, EXACT, seam=odd_seam(n))
    splits = mfma_splits(n, nq, 32)
    assert set(ran) == {MFMA} and last[0] == 0, ran
    assert ran[MFMA] == [((-(-nq // 32) * splits, 1, 1), 256, 32 * (D + 16))], (ran, splits)
    assert splits == {10241: 5, 16384 + 77: 8}.get(n, 1)
    check(d, i, db, q, k, (n, D, nq, k))


@gpu
@pytest.mark.parametrize("D", [128, 160])
def test_mfma_kernel_every_row_beats_the_threshold(amd, D):
    """2000 rows sorted by decreasing distance to query 0, k = 128: every row is better than all before it, the 208-entry buffer fills past
    its trigger tile after tile and the `pending` loop has to re-offer what a full buffer turned away; the other queries see the rows
    in no order"""
    n, nq, k = 2000, 5, 128
    db, q = table(D, n, D, nq)
    x = db.astype(np.int64) - q[0].astype(np.int64)
    db = np.ascontiguousarray(db[np.argsort(-(x * x).sum(axis=1), kind="stable")])
    d, i, ran, last = search(amd, db, q, k, EXACT)
    assert set(ran) == {MFMA} and ran[MFMA] == [((1, 1, 1), 256, 32 * (D + 16))], ran
    check(d, i, db, q, k, D)
    assert i[0].min() >= n - 3 * k                            # query 0's neighbours come from the end of the table


# ---- the row-tile kernels: flat_u8_rowtile_kernel<NW, CAP, DMAX, OPT> ----

ROWTILE_CASES = [  # (n, D, nq, k, NW, what)
    (5000, 64, 33, 10, 2, ""), (5000, 256, 64, 24, 2, ""),                        # NW 2: 33 .. 64 queries, k <= 24; one split
    (5000 + 13, 128, 65, 1, 4, ""), (24_621, 512, 128, 12, 4, ""),                # NW 4: 65 .. 128 queries; one past a tile; 3 splits, a partial last tile
    (5000, 96, 129, 24, 8, ""), (24_621, 256, 257, 5, 8, ""),                     # NW 8: > 128 queries; one past one / two tiles of 128
    (5000, 128, 65, 25, 4, ""), (24_621, 160, 129, 80, 4, ""), (8192 * 2, 32, 300, 33, 4, ""),   # CAP 112: 25 <= k <= 80 with more than 64 queries
    (16_384, 128, 65, 1, 4, "slots"), (49_152 + 31, 64, 129, 3, 8, "slots"), (262_144, 32, 33, 16, 2, "slots"),   # nslot > 0: k <= 16 and splits >= 2 k
    (24_621, 128, 65, 10, 4, "equal"), (16_384, 256, 33, 1, 2, "equal slots"), (49_152, 32, 257, 3, 8, "equal slots"),   # every row the same
    (40_000, 128, 65, 10, 4, "kth"), (40_000, 64, 33, 3, 2, "kth"),               # the k-th best again in the first and in the last split
    (40_000, 128, 65, 10, 4, "late tie"), (40_000, 256, 129, 24, 8, "late tie"),  # a row deep in the first split that ties the k-th best another split has published
    (16_384, 128, 65, 1, 4, "slots tie"), (49_152 + 31, 64, 129, 3, 8, "slots tie"), (262_144, 32, 33, 16, 2, "slots tie")]   # ... or the largest of the k slot minima


@gpu
@pytest.mark.parametrize("n,D,nq,k,nw,what", ROWTILE_CASES)
def test_rowtile_kernels(amd, n, D, nq, k, nw, what):
    qt = mfma_qtile(D, k, nq)
    assert qt > 32 and nw == {64: 2, 128: 4, 256: 8}[qt if k <= 24 else 128]
    db, q = table(n + D * 3 + nq + k, n, D, nq)
    splits = mfma_splits(n, nq, qt)
    if "equal" in what:       # rows 0 .. k - 1 win on the row alone, whatever bound the other splits publish
        db[:] = db[0]
    rps = -(-(-(-n // splits)) // 128) * 128   # rows per split: whole 128-row units (launch_flat_u8_mfma)
    if "late" in what or "slots tie" in what:
        # Copies of query 0 (distance 0) at the head of later splits, which publish them at once, and one more near the END of the first
        # split, met long after: it ties the shared bound and wins on its row, so the `+ 1` on that bound has to let it through.
        # "late tie": the last split opens with k copies -- its own k-th best, gthr, is 0.  "slots tie": each of the last k splits opens
        # with ONE copy -- the k slots (split % k), gslot, all hold 0 while no split's k-th best does (k > 1).
        q[0] = np.random.default_rng(n + k).integers(0, 256, size=D, dtype=np.uint8)
        if "late" in what:
            db[(splits - 1) * rps:(splits - 1) * rps + k] = q[0]
        else:
            db[np.arange(splits - k, splits) * rps] = q[0]
        db[rps - 100] = q[0]
    if "kth" in what:         # query 0's k-th best once more near the start and near the end
        _, mi = model(db, q[:1], k)
        db[7] = db[mi[0, k - 1]]; db[n - 3] = db[mi[0, k - 1]]
    d, i, ran, last = search(amd, db, q, k, EXACT, seam=odd_seam(n))
    assert set(ran) == {ROWTILE} and last[0] == 0, ran
    assert ran[ROWTILE] == [((-(-nq // qt) * splits, 1, 1), 64 * nw, 2 * 32 * (D + 16))], (ran, splits)
    assert (splits >= 2 * k and k <= 16) == ("slots" in what) and (splits > 1 or n < 16_384)
    check(d, i, db, q, k, (n, D, nq, k, what))
    if "equal" in what:
        assert np.array_equal(i, np.tile(np.arange(k), (nq, 1)))


@gpu
@pytest.mark.parametrize("opt", [1, 2, 3])
def test_rowtile_kernel_operand_forms(amd, opt):
    """flat_u8_opt 1 .. 3: the other forms of the 8-wave kernel for D > 128 (two accumulator chains, operands read ahead) -- same lists"""
    n, D, nq, k = 24_621, 512, 257, 5
    db, q = table(opt, n, D, nq)
    d, i, ran, _ = search(amd, db, q, k, dict(EXACT, flat_u8_opt=opt), seam=odd_seam(n))
    assert set(ran) == {ROWTILE} and ran[ROWTILE] == [((2 * 3, 1, 1), 512, 2 * 32 * (D + 16))], ran
    check(d, i, db, q, k, opt)


# ---- the stream and its selection: flat_u8_mstream_kernel<KS, QB> + flat_u8_stream_finish_kernel ----

STREAM_CASES = [  # (n, D, nq, k): QB 1 / 2 / 4 with padding queries, two balanced passes; 4096 rows: exactly 128 waves hold a tile
    (4096, 128, 1, 1), (4096, 256, 32, 128), (4097, 512, 33, 10), (4128, 128, 64, 128), (4097, 256, 65, 10), (4128, 512, 128, 1), (4096, 128, 129, 128),
    (4096, 512, 3, 128), (4128, 256, 129, 1),
    (32 * (4 * 1024 + 300) - 13, 128, 33, 10),      # 4396 tiles over 1024 waves: 300 waves hold five, the others four -- their second group of four is partial
    (32 * (8 * 1024 + 1) - 13, 256, 7, 10)]         # one wave with a third group of a single tile, cut short


@gpu
@pytest.mark.parametrize("n,D,nq,k", STREAM_CASES)
def test_stream_and_finish(amd, n, D, nq, k):
    db, q = table(n + D + nq * 3 + k, n, D, nq)
    d, i, ran, last = search(amd, db, q, k, STREAMED, seam=odd_seam(n))
    passes = -(-nq // 128)
    per = -(-nq // passes)
    sizes = [min(per, nq - a) for a in range(0, nq, per)]
    assert set(ran) == set(STREAM) and last[0] == 0, ran
    assert [(g, b) for g, b, _ in ran[STREAM[0]]] == [((256, 1, 1), 256)] * passes
    assert [(g, b) for g, b, _ in ran[STREAM[1]]] == [((m * stream_slices(m), 1, 1), 256) for m in sizes], (ran, sizes)
    check(d, i, db, q, k, (n, D, nq, k))


@gpu
@pytest.mark.parametrize("planted", [False, True])
def test_stream_finish_slice_full_of_tiles_under_theta(amd, planted):
    """The finish kernel's `n_cl > FIN_CL` fallback: every row at the same distance, so every wave minimum equals theta and every chunk of
    32 rows qualifies.  65 .. 128 queries get S = 8 slices; a slice lists at most FIN_CL = 1024 chunks, and 8 x 1024 + 1 = 8193 chunks
    -- 262 145 rows, the last chunk a single row -- give the last slice 1025.  The lists are analytic: rows 0 .. k - 1, and with one nearer
    row planted in that last slice, that row and then rows 0 .. k - 2.  (Only the planted row comes out of the fallback here; the next test
    makes the whole list do so.)"""
    n, D, nq, k = 32 * 8 * 1024 + 1, 128, 128, 10
    chunks = -(-n // 32)
    assert max(chunks * (s + 1) // 8 - chunks * s // 8 for s in range(8)) == 1025 and chunks * 7 // 8 == 7168
    assert max((chunks - 1) * (s + 1) // 8 - (chunks - 1) * s // 8 for s in range(8)) == 1024      # one chunk fewer: no slice over FIN_CL
    rng = np.random.default_rng(5)
    row = rng.integers(0, 256, size=D, dtype=np.uint8)
    db = np.tile(row, (n, 1))
    q = rng.integers(0, 256, size=(nq, D), dtype=np.uint8)
    q[3] = row
    near = n - 40                                            # (chunk 8190: inside the last slice, not its last chunk)
    if planted:                                              # every byte one step towards the mean query
        db[near] = (row.astype(np.int32) + np.sign(q.astype(np.int32).sum(axis=0) - nq * row.astype(np.int32))).clip(0, 255).astype(np.uint8)
    d, i, ran, last = search(amd, db, q, k, STREAMED, seam=odd_seam(n))
    assert set(ran) == set(STREAM) and ran[STREAM[1]][0][0] == (nq * 8, 1, 1), ran
    common = model(db[:1], q, 1)[0][:, 0]                     # the one distance of a query to every other row (the model on that row alone)
    want_i = np.tile(np.arange(k), (nq, 1))
    want_d = np.tile(common[:, None], (1, k))
    if planted:
        pd = model(db[near:near + 1], q, 1)[0][:, 0]
        closer = pd < common                                  # (a tie loses to rows 0 .. k - 1 on the row number)
        assert closer.sum() > nq // 2 and not closer[3]
        want_i[closer] = np.concatenate([[near], np.arange(k - 1)])
        want_d[closer, 0] = pd[closer]
    assert np.array_equal(i, want_i) and np.array_equal(d, want_d), np.flatnonzero(np.any(i != want_i, axis=1) | np.any(d != want_d, axis=1))[:8]


@gpu
@pytest.mark.parametrize("planted", [False, True])
def test_stream_finish_full_slice_answers(amd, planted):
    """The same shape, but the answer has to come OUT of the slice that takes the fallback (above, rows 0 .. k - 1 belong to the first
    slice, which lists 1024 chunks and takes the usual path): the rows of the last slice -- chunks 7168 .. 8192 -- are one vector near
    every query, all rows before them one far vector.  Every wave holds a tile of the last slice, so every wave minimum is theta and
    all of the slice's 1025 chunks are under it; the expected lists are its first k rows, or a planted nearer row and its first k - 1."""
    n, D, nq, k = 32 * 8 * 1024 + 1, 128, 128, 10
    first = 7168 * 32
    rng = np.random.default_rng(6)
    row = rng.integers(0, 250, size=D, dtype=np.uint8)
    db = np.empty((n, D), np.uint8)
    db[:first] = 255 - row
    db[first:] = row
    q = (row[None, :] + rng.integers(0, 3, size=(nq, D))).astype(np.uint8)     # each byte 0 .. 2 above the near vector
    q[3] = row
    near = n - 40
    if planted:
        db[near] = row + 1
    d, i, ran, last = search(amd, db, q, k, STREAMED, seam=odd_seam(n))
    assert set(ran) == set(STREAM) and ran[STREAM[1]][0][0] == (nq * 8, 1, 1), ran
    common = model(db[first:first + 1], q, 1)[0][:, 0]
    assert np.all(common < model(db[:1], q, 1)[0][:, 0])
    want_i = np.tile(first + np.arange(k), (nq, 1))
    want_d = np.tile(common[:, None], (1, k))
    if planted:
        pd = model(db[near:near + 1], q, 1)[0][:, 0]
        closer = pd < common
        assert closer.sum() > nq // 2 and not closer[3]
        want_i[closer] = np.concatenate([[near], first + np.arange(k - 1)])
        want_d[closer, 0] = pd[closer]
    assert np.array_equal(i, want_i) and np.array_equal(d, want_d), np.flatnonzero(np.any(i != want_i, axis=1) | np.any(d != want_d, axis=1))[:8]


# ---- the sample + filter pipeline: flat_variant 2 ----

PIPE_CASES = [  # (n, D, nq, k, tune, sample kernels, filter kernel): a 65 536-row sample, then the packed rows from there on -- the pack's last tile full / 1 / 31 rows
    (131_072, 128, 40, 10, {}, STREAM, "flat_u8_gfilter_kernel"),
    (131_073, 128, 40, 10, {}, STREAM, "flat_u8_gfilter_kernel"),
    (131_103, 256, 130, 64, {}, STREAM, "flat_u8_gfilter_kernel"),
    (131_072, 512, 40, 10, {}, STREAM, "flat_u8_gfilter_kernel"),
    (131_073, 64, 40, 10, {}, (ROWTILE,), "flat_u8_gfilter_kernel"),                                # widths without a stream: the sample through a row-tile kernel
    (131_103, 96, 40, 10, {}, (ROWTILE,), "flat_u8_filter_kernel"),
    (131_073, 128, 20, 33, dict(flat_u8_sample_passes=0), (MFMA,), "flat_u8_gfilter_kernel")]         # the sample past flat_u8_sample_passes: the exact kernels


@gpu
@pytest.mark.parametrize("n,D,nq,k,tune,sample,filt", PIPE_CASES)
def test_pipeline(amd, n, D, nq, k, tune, sample, filt):
    db, q = table(n + D + nq + k, n, D, nq)
    db[65_535] = db[9]; db[65_536] = db[9]; q[1] = db[9]       # the same row on both sides of the sample's end
    d, i, ran, last = search(amd, db, q, k, dict(PIPELINE, **tune), seam=odd_seam(n))
    assert set(ran) == {*sample, filt, *PIPE_FINISH}, ran
    cap = min(4096 - k, (48 * k + 1024 + 63) // 64 * 64)
    assert last[0] == 1 and 0 < last[1] <= cap, last
    check(d, i, db, q, k, (n, D, nq, k))
    assert i[1, :3].tolist() == [9, 65_535, 65_536]


@gpu
def test_pipeline_candidate_lists_overflow(amd):
    """bytes in 0 .. 3; the sample's rows far from every query, every row behind it near: all 65 600 of them pass the sample's threshold,
    the candidate lists (1536 entries at k = 10) run over, and the exact path -- here the stream -- answers the call"""
    n, D, nq, k = 131_072 + 64, 128, 40, 10
    rng = np.random.default_rng(9)
    db = rng.integers(2, 4, size=(n, D), dtype=np.uint8)
    db[65_536:] = rng.integers(0, 2, size=(n - 65_536, D), dtype=np.uint8)
    q = rng.integers(0, 2, size=(nq, D), dtype=np.uint8)
    db[n - 1] = db[70_000]; q[0] = db[70_000]
    d, i, ran, last = search(amd, db, q, k, PIPELINE)
    cap = min(4096 - k, (48 * k + 1024 + 63) // 64 * 64)
    assert cap == 1536 and last[0] == 0 and last[1] > cap, last
    assert set(ran) == {*STREAM, "flat_u8_gfilter_kernel", *PIPE_FINISH} and len(ran[STREAM[0]]) == 2, ran   # the sample's pass and the answer's
    check(d, i, db, q, k, "overflow")


# ---- the threshold filter (its own tests: test_gpu_flat_sq8.py): the route alone ----

@gpu
def test_threshold_filter_route(amd):
    n, D, nq, k = 65_536, 128, 129, 10
    db, q = table(77, n, D, nq)
    d, i, ran, last = search(amd, db, q, k, dict(flat_variant=0), seam=odd_seam(n))
    assert set(ran) == {*TFILTER, DOT4} and last[0] == 4, ran   # (the dot4 kernel: the predicated re-run of flagged queries, which exits at once without any)
    assert len(ran[TFILTER[0]]) == 2                            # the sample pass and the filter pass
    check(d, i, db, q, k, "tfilter")
    d2, i2, ran2, last2 = search(amd, db, q[:128], k, dict(flat_variant=0))   # one query fewer: a stream pass
    assert set(ran2) == set(STREAM) and last2[0] == 0, ran2
    assert np.array_equal(d2, d[:128]) and np.array_equal(i2, i[:128])
    d3, i3, ran3, _ = search(amd, db, q, k, dict(flat_variant=0, flat_u8_mstream_min=129, flat_u8_tfilter=0))   # both off: a row-tile kernel
    assert set(ran3) == {ROWTILE} and ran3[ROWTILE][0][1] == 64 * 8, ran3
    assert np.array_equal(d3, d) and np.array_equal(i3, i)
