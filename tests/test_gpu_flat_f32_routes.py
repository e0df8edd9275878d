"""The exact fp32 flat-search kernels by name -- flat_f32_kernel (row-major rows, queries in LDS: D % 4 != 0) and flat_f32_sq_kernel
(64-row blocked rows, queries in SGPRs: D % 4 == 0) with flat_block_kernel / flat_unblock_kernel around them -- at their width, tile,
block, split and tie edges.  The rest of the suite takes these kernels as ground truth ("same as flat_variant 1"), they answer every
query a filter flags (the `only_if` predicate) and every width, table and k the faster routes leave; cvtmi_flat_last_search reports 0
whichever of them ran, so every case here reads the launch log (cvt_amd.launch_log) and asserts the kernel it was shaped for, its grid
(query groups x row splits, the splits from a host copy of flat_plan_splits), its block, its dynamic LDS, and that no other fp32 search
kernel ran.

The reference is a numpy model of the operation, not another kernel: the distance in the reference's own summation order (IP = 1 - sum
in 4 lanes when D % 4 == 0; L2F in 8 lanes when D % 16 == 0, in 4 when D % 4 == 0; the scalar loop otherwise), every step a separate
fp32 numpy operation (acc[l] += q[i + l] * x[i + l], lanes summed left to right: nothing is contracted), ranked by a stable order on
(f32_key of the distance bits, row), padded with label -1 and the bits 0x7f800000.  Every query of every case is compared, distance bits
and labels, exactly.  One CPU test checks the model itself against the oracle.

Every table holds one row three times (ties on (distance, row), asked for by query 0), a zero row, rows scaled by 1e-25 (query 1 is one
of them: under IP every row but one is then at distance exactly 1, under L2F the tiny rows and the zero row tie at +0), one element
of 3e19 (its square overflows: a +inf L2F distance is a real candidate) and, for IP, negative distances."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

gpu = pytest.mark.gpu
IP, L2F = 0, 1
PAD = 0x7f800000

SQ, LDSQ = "flat_f32_sq_kernel", "flat_f32_kernel"
BLOCK, UNBLOCK = "flat_block_kernel", "flat_unblock_kernel"
TFILTER = ("flat_f32_tfilter_kernel", "ft_theta_kernel", "ft_bucket_kernel", "ft_finish_kernel")
# every kernel that computes or selects fp32 distances for a search (flat.hip, flat_f32_stream.hip, flat_f32_tfilter.hip, flat_mfma.hip);
# the layout / operand-copy / merge / label kernels around them are not routes
F32_SEARCH = {SQ, LDSQ, *TFILTER, "ft_finish_big_kernel", "flat_f32_mstream_kernel", "flat_f32_mshare_kernel", "flat_f32_stream_collect_kernel",
              "flat_f32_stream_finish_kernel", "flat_thr_kernel", "flat_filter_kernel", "flat_scatter_kernel", "flat_finish_kernel"}
EXACT = dict(flat_variant=1)


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()
    return cvt_amd


# ---- the model ----

def lanes_of(metric, D):
    if D % 4:
        return 1
    return 8 if metric == L2F and D % 16 == 0 else 4


def distances(metric, db, q):
    """fp32 [nq][n]: every (query, row) distance in the reference's summation order, one fp32 numpy operation per step"""
    n, D = db.shape
    L = lanes_of(metric, D)
    acc = np.zeros((q.shape[0], n, L), np.float32)
    with np.errstate(all="ignore"):
        for i in range(0, D, L):
            a, x = q[:, None, i:i + L], db[None, :, i:i + L]
            if metric == IP:
                acc += a * x
            else:
                t = a - x
                acc += t * t
        s = acc[:, :, 0].copy()
        for l in range(1, L):
            s = s + acc[:, :, l]
        if metric == IP:
            s = np.float32(1.0) - s
    assert s.dtype == np.float32
    return s


def f32_key(b):
    """common.h: the order-preserving uint32 key of a float's bits"""
    b = np.ascontiguousarray(b, np.uint32)
    return b ^ ((b.view(np.int32) >> 31).view(np.uint32) | np.uint32(0x80000000))


def ranking(dist_row):
    """the rows of one query in the stable order on (f32_key of the distance bits, row)"""
    key = (f32_key(dist_row.view(np.uint32)).astype(np.uint64) << np.uint64(32)) | np.arange(dist_row.shape[0], dtype=np.uint64)
    return np.argsort(key, kind="stable")


def model(metric, db, q, k):
    """(distance bits uint32 [nq][k], rows int64 [nq][k]) of the k nearest rows"""
    dist = distances(metric, db, q)
    nq, n = dist.shape
    kk = min(k, n)
    bits = np.full((nq, k), PAD, np.uint32)
    rows = np.full((nq, k), -1, np.int64)
    for j in range(nq):
        order = ranking(dist[j])[:kk]
        rows[j, :kk] = order
        bits[j, :kk] = dist[j].view(np.uint32)[order]
    return bits, rows


def table(seed, metric, n, D, nq, third=None):
    """the common ingredients (module docstring); the third copy of row 2 goes to row `third` (the last row by default)"""
    rng = np.random.default_rng(seed)
    db = rng.normal(size=(n, D)).astype(np.float32)
    q = rng.normal(size=(nq, D)).astype(np.float32)
    if n >= 26:
        if metric == IP:       # every element 1.5 or more in magnitude: 1 - |x|^2 < 0
            db[2] = np.copysign(np.float32(1.5) + np.abs(db[2]), db[2])
        db[n // 2] = db[2]; db[n - 1 if third is None else third] = db[2]; q[0] = db[2]
        db[5] = 0
        db[7:10] *= np.float32(1e-25)
        db[11, D // 2] = np.float32(3e19)
        if nq > 1:
            q[1] = db[8]
    return db, q


def specials(n, third=None):
    return {2, n // 2, n - 1 if third is None else third, 5, 7, 8, 9, 11} if n >= 26 else set()


SMALL = [(1, 1, 1), (2, 3, 5), (40, 5, 8), (300, 16, 40), (129, 21, 129), (64, 32, 10), (65, 36, 2048), (1025, 48, 100), (513, 128, 5),
         (100, 4095, 7), (26, 4, 30), (700, 7, 2048)]


@pytest.mark.parametrize("metric", [IP, L2F])
@pytest.mark.parametrize("n,D,k", SMALL)
def test_model_equals_the_oracle(orc, metric, n, D, k):
    """the numpy model against the CPU oracle's loops on small tables -- every lane order, the scalar loop up to 4095 dimensions,
    duplicates, tiny rows, the 3e19 element, the zero row, k above the row count -- so that the GPU cases below rest on a reference
    checked without a GPU"""
    nq = 3
    db, q = table(n * 31 + D + metric, metric, n, D, nq)
    od, _, oi = orc.flat_search(metric, db, q, k)
    mb, mi = model(metric, db, q, k)
    assert np.array_equal(mi, oi) and np.array_equal(mb, np.ascontiguousarray(od).view(np.uint32))
    if k > n:
        assert np.all(mi[:, n:] == -1) and np.all(mb[:, n:] == PAD)
    if n >= 26 and metric == IP:
        assert np.any(mb.view(np.float32)[mi >= 0] < 0)
    if n >= 26 and metric == L2F:
        assert mi[0, :min(k, 3)].tolist() == [2, n // 2, n - 1][:min(k, 3)] and np.all(mb[0, :min(k, 3)] == 0)   # the three copies at distance +0
        if k >= n:
            assert np.any(mb[mi >= 0] == PAD)                    # the overflowed row: +inf with a label


# ---- host models of the planners (cvt_amd/csrc/flat.hip, api_flat.hip), to derive shapes and to read split counts off the grid ----

def plan_splits(n, nq, qt):                                       # flat_plan_splits
    groups = -(-nq // qt)
    return max(1, min(2048 // groups, max(n // 2048, 1), 1024))


def qtile(nq, k):                                                 # flat_search_rows: k > 128 takes one query per workgroup
    return 1 if k > 128 or nq < 4 else 4


def rows_per_split(n, splits):                                    # launch_flat_search: whole 512-row tiles
    return max(512, -(-(-(-n // splits)) // 512) * 512)


def instance(metric, D, nq, k):
    """the template instance launch_f32 picks: (IP, LANES, QT or "big")"""
    return ("IP" if metric == IP else "L2F", lanes_of(metric, D), "big" if k > 128 else qtile(nq, k))


# ---- running a case ----

@contextlib.contextmanager
def tuned(amd, **keys):
    old = {name: amd.get_tuning(name) for name in keys}
    try:
        for name, value in keys.items():
            amd.set_tuning(name, value)
        yield
    finally:
        for name, value in old.items():
            amd.set_tuning(name, value)


def searched(log):
    ran = {}
    for name, grid, block, lds in log:
        if name in F32_SEARCH:
            ran.setdefault(name, []).append((grid, block, lds))
    return ran


def odd_seam(n):
    return (n // 2) | 1 if n > 2 else None                        # two appends whose seam is no multiple of 64 (nor of anything even)


def search(amd, metric, db, q, k, seam=None):
    """the search under flat_variant 1 -> (distances, labels, {kernel name: [(grid, block, lds), ...]} of the fp32 search kernels, last_search())"""
    with tuned(amd, **EXACT):
        ix = amd.FlatIndex(metric, db.shape[1])
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
    return d, i, searched(log), last


def expect_exact(ran, last, n, D, nq, k):
    """the one exact kernel of the shape, its grid, block and dynamic LDS; -> (qt, splits)"""
    qt = qtile(nq, k)
    splits = plan_splits(n, nq, qt)
    name = SQ if D % 4 == 0 else LDSQ
    assert set(ran) == {name} and last[0] == 0, (ran, last)
    assert ran[name] == [((-(-nq // qt) * splits, 1, 1), 256, 0 if name == SQ else qt * D * 4)], (ran, qt, splits)
    return qt, splits


def check(metric, d, i, db, q, k, what, labels=None):
    mb, mi = model(metric, db, q, k)
    if labels is not None:
        mi = np.where(mi >= 0, labels[np.maximum(mi, 0)], -1)
    b = np.ascontiguousarray(d).view(np.uint32)
    bad = np.flatnonzero(np.any(i != mi, axis=1) | np.any(b != mb, axis=1))
    assert d.dtype == np.float32 and bad.size == 0, (what, "queries", bad[:8].tolist(), i[bad[:1]].tolist(), mi[bad[:1]].tolist(), b[bad[:1]].tolist(), mb[bad[:1]].tolist())
    return mb, mi


def exact_case(amd, metric, n, D, nq, k, db=None, q=None):
    if db is None:
        db, q = table(n * 7 + D * 3 + nq + k + metric, metric, n, D, nq)
    d, i, ran, last = search(amd, metric, db, q, k, seam=odd_seam(n))
    qt, splits = expect_exact(ran, last, n, D, nq, k)
    mb, mi = check(metric, d, i, db, q, k, (metric, n, D, nq, k))
    if metric == IP and n >= 26:
        assert np.any(mb.view(np.float32)[mi >= 0] < 0)
    return splits, mb, mi


# ---- 1. widths and lane orders ----

WIDTHS = [1, 2, 3, 5, 7, 21, 4095,      # the scalar loop over row-major rows: flat_f32_kernel
          4, 12, 20, 36,                # 4 lanes
          16, 48, 128,                  # 8 lanes for L2F, 4 for IP
          4096]                         # the widest row


@gpu
@pytest.mark.parametrize("metric", [IP, L2F])
@pytest.mark.parametrize("nq", [3, 5])
@pytest.mark.parametrize("D", WIDTHS)
def test_widths_and_lane_orders(amd, metric, D, nq):
    """nq 3: QT 1, nq 5: QT 4 with three clamped padding queries.  D = 4095 at nq = 5 asks for 4 x 4095 x 4 = 65 520 bytes of dynamic
    LDS next to the static selection buffers of four queries (about 12 KB): more than 64 KB in all, through a plain launch() -- measured:
    the runtime takes the launch (a gfx950 workgroup may hold 160 KB) and the lists are exact"""
    splits, _, _ = exact_case(amd, metric, 513, D, nq, 5)
    assert splits == 1


# ---- 2. query tiles and selection buffers ----

@gpu
@pytest.mark.parametrize("metric", [IP, L2F])
@pytest.mark.parametrize("D", [21, 32])
@pytest.mark.parametrize("nq", [1, 3, 4, 5, 7])
def test_query_tiles(amd, metric, D, nq):
    """QT 1 (nq < 4) and QT 4 with 0 .. 3 clamped padding queries"""
    exact_case(amd, metric, 1000, D, nq, 10)


SELECTION_D = [21, 32, 36]
SELECTION = [(3000, 5, 1), (3000, 5, 128), (3000, 5, 129), (3000, 5, 2048), (511, 2, 2048), (52, 5, 128)]


def test_cases_reach_every_template_instance():
    """host logic: the shapes of cases 1 and 2 instantiate, by launch_f32's rule, all 15 of {IP LANES 1 / 4, L2F LANES 1 / 4 / 8} x
    {QT 1, QT 4, the kBigCap instance} -- the launch log names the kernel, not its template arguments"""
    reached = {instance(m, D, nq, 5) for m in (IP, L2F) for D in WIDTHS for nq in (3, 5)}
    assert len(reached) == 10
    reached |= {instance(m, D, nq, k) for m in (IP, L2F) for D in SELECTION_D for _, nq, k in SELECTION}
    assert reached == {(m, lanes, t) for m, ls in (("IP", (1, 4)), ("L2F", (1, 4, 8))) for lanes in ls for t in (1, 4, "big")}


@gpu
@pytest.mark.parametrize("metric", [IP, L2F])
@pytest.mark.parametrize("D", SELECTION_D)
@pytest.mark.parametrize("n,nq,k", SELECTION)
def test_selection_buffers(amd, metric, D, n, nq, k):
    """k on both sides of 128 (the 384-entry buffers of four queries / the 4096-entry buffer of one) and above the row count; the three
    widths reach the kBigCap instance of every (metric, lanes) pair"""
    _, mb, mi = exact_case(amd, metric, n, D, nq, k)
    if k > n:
        assert np.all(mi[:, n:] == -1) and np.all(mi[:, :n] >= 0)


# ---- 3. rows around the tile and the block ----

@gpu
@pytest.mark.parametrize("metric", [IP, L2F])
@pytest.mark.parametrize("D", [32, 5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 511, 512, 513])
def test_rows_around_the_tile_and_the_block(amd, metric, D, n):
    """a row; one short of a 64-row block, the block, one past it; the same around the 512-row tile"""
    exact_case(amd, metric, n, D, 4, 10)


# ---- 4. split plans ----

@gpu
@pytest.mark.parametrize("metric", [IP, L2F])
@pytest.mark.parametrize("D,k", [(128, 10), (21, 10), (128, 129), (21, 129)])
@pytest.mark.parametrize("nq", [1, 7])
@pytest.mark.parametrize("n", [12289, 10241])
def test_split_plans(amd, metric, n, nq, D, k):
    """n // 2048 splits of whole 512-row tiles: 6 x 2560 -- the sixth starts at row 12 800, past the table; 5 x 2560 -- the fifth holds
    row 10 240 alone"""
    splits, _, _ = exact_case(amd, metric, n, D, nq, k)
    rps = rows_per_split(n, splits)
    assert splits == n // 2048 and n - (splits - 1) * rps == (1 if n == 10241 else -511)


@gpu
@pytest.mark.parametrize("metric", [IP, L2F])
def test_split_plans_rows_decide_across_the_merge(amd, metric):
    """the best row of query 3 again in a middle split and in the last split that holds rows: three equal distances from three partial
    lists, ordered by row in the merge"""
    n, D, nq, k = 12289, 128, 7, 10
    db, q = table(99 + metric, metric, n, D, nq)
    best = int(model(metric, db, q[3:4], 1)[1][0, 0])
    rps = rows_per_split(n, plan_splits(n, nq, 4))
    assert rps == 2560 and len({best // rps, 6000 // rps, 12000 // rps}) == 3 and best not in (2, n // 2, n - 1)
    db[6000] = db[best]; db[12000] = db[best]
    _, _, mi = exact_case(amd, metric, n, D, nq, k, db, q)
    assert mi[3, :3].tolist() == sorted([best, 6000, 12000])


# ---- 5. the blocked layout under appends ----

APPENDS = ["host", "host labels", "host one by one", "device", "device id_base", "device off 16 bytes"]


def append_table(metric, D, n):
    """the common table with the third copy three rows before the end; under IP a row is its own nearest neighbour only if nothing longer
    points its way: the ordinary rows are four times as long as drawn and negative in the column of the 3e19 element"""
    third = n - 3
    db, _ = table(500 + D + metric, metric, n, D, 1, third=third)
    ordinary = set(range(n)) - specials(n, third)
    if metric == IP:
        o = np.array(sorted(ordinary))
        db[o] *= np.float32(4.0)
        db[o, D // 2] = -np.abs(db[o, D // 2])
    return db, ordinary


@gpu
@pytest.mark.parametrize("metric", [IP, L2F])
@pytest.mark.parametrize("D", [32, 128])
@pytest.mark.parametrize("how", APPENDS)
def test_blocked_layout_under_appends(amd, metric, D, how):
    """flat_block_kernel writes at row0 = ntotal into whole 64-row blocks.  1000 + 100 + 1 rows: no seam on a multiple of 64, and the
    second append crosses the first capacity of 1024 rows from inside a half-filled block; 70 appends of one row fill a block and start
    the next.  Host rows are staged, a 16-byte-aligned device pointer is read in place, a device pointer one float off 16 bytes is staged.
    After every append rows from before, at and after each seam are searched for: each comes back first, every list equals the model"""
    import torch
    pieces = [1] * 70 if "one by one" in how else [1000, 100, 1]
    n_all = sum(pieces)
    db, ordinary = append_table(metric, D, n_all)
    labels = np.arange(n_all, dtype=np.int64) * 3 + 5 if "labels" in how else None
    base = 1000 if "id_base" in how else 0
    k = 5
    keep = []
    with tuned(amd, **EXACT):
        ix = amd.FlatIndex(metric, D)
        try:
            if base:
                ix.set_id_base(base)
            n = 0
            seams = []
            for p in pieces:
                piece = db[n:n + p]
                if "device" in how:
                    if "off" in how:
                        buf = torch.empty(p * D + 1, dtype=torch.float32, device="cuda")
                        buf[1:] = torch.from_numpy(piece).reshape(-1)
                        x = buf[1:].view(p, D)
                        assert x.data_ptr() % 16 == 4
                    else:
                        x = torch.from_numpy(piece).cuda()
                        assert x.data_ptr() % 16 == 0
                    keep.append(x)
                else:
                    x = piece
                with amd.launch_log() as log:
                    ix.add(x, labels=None if labels is None else labels[n:n + p])
                assert [(g, b) for name, g, b, _ in log if name == BLOCK] == [((min(-(-p * (D // 4) // 256), 256 * 64), 1, 1), 256)], log
                seams.append(n)
                n += p
                assert ix.ntotal == n
                around = {0, 1, 62, 63, 64, 65, n - 2, n - 1, n // 2 + 1}
                for s in seams:
                    around |= {s - 2, s - 1, s, s + 1}
                rows = np.array(sorted(r for r in around if 0 <= r < n and r in ordinary))   # (row 0 is ordinary: never empty)
                q = np.ascontiguousarray(db[rows])
                with amd.launch_log() as log:
                    d, i = ix.search(q, k)
                expect_exact(searched(log), ix.last_search(), n, D, len(rows), k)
                want = None if labels is None and not base else (labels if labels is not None else np.arange(n_all, dtype=np.int64) + base)
                _, mi = check(metric, d, i, db[:n], q, k, (how, n), labels=want)
                first = rows if want is None else want[rows]
                assert np.array_equal(mi[:, 0], first) and np.array_equal(i[:, 0], first), (how, n)
            torch.cuda.synchronize()
        finally:
            ix.close()


# ---- 6. the predicated re-run against the model ----

HARD_N1, HARD_N, HARD_D, HARD_NQ, HARD_K = 32768 + 5, 32768 + 77, 32, 18, 10
HARD_TUNE = dict(flat_variant=0, flat_f32_tfilter_min=16, flat_f32_tfilter_min_rows=32768, flat_count_redo=1)


@functools.lru_cache(maxsize=None)
def hard_table(metric):
    """Queries in groups of four: 0 .. 3 the common ones (query 1, a 1e-25 row, is below the magnitudes the filter's bound covers), 4 .. 7
    with query 5 scaled by 2^70 (one flagged query of four), 8 .. 11 a zero query, a query tied by 3001 equal rows at the k-th place, one
    scaled by 2^70 and one by -2^61 (four of four), 12 .. 15 ordinary (no flagged query), 16 and 17 with two clamped padding queries
    behind them, 17 scaled by 2^70.  (Under L2F a 2^70 query is at +inf from every row: rows 0 .. k - 1 win on the row alone.)
    Of the common ingredients the 3e19 element is left out: its square overflows, the row statistics count that as a non-finite row, and
    a table with one never takes the filter (it goes to the exact kernels whole: cases 1 .. 5 have that)."""
    n, D, nq = HARD_N, HARD_D, HARD_NQ
    db, q = table(600 + metric, metric, n, D, nq)
    db[11, D // 2] = np.float32(0.25)
    db[3000:6000] = db[20]
    q[9] = db[20]
    q[8] = 0
    q[5] *= np.float32(2.0 ** 70); q[10] *= np.float32(2.0 ** 70); q[17] *= np.float32(2.0 ** 70)
    q[11] *= np.float32(-2.0 ** 61)
    db.setflags(write=False); q.setflags(write=False)
    return db, q, model(metric, db[:HARD_N1], q, HARD_K), model(metric, db, q, HARD_K)


def describe_dispatch(amd, metric, D, n, nq, k):
    out = (C.c_int * 4)()
    assert amd.lib().cvtmi_flat_describe_dispatch(metric, D, C.c_int64(n), C.c_int64(nq), k, out) == 0
    return list(out)


@pytest.mark.parametrize("metric", [IP, L2F])
def test_predicated_rerun_shape_takes_the_threshold_filter(metric):
    """host logic, no device: flat_f32_tfilter_applies takes both states of the case-6 table under its tuning (D % 4 == 0 up to 2048,
    n at the floor of "flat_f32_tfilter_min_rows", nq at "flat_f32_tfilter_min", k <= 128, the sample's slots filled) and not one row below the floor"""
    import cvt_amd
    keys = {name: value for name, value in HARD_TUNE.items() if name != "flat_count_redo"}
    with tuned(cvt_amd, **keys):
        assert describe_dispatch(cvt_amd, metric, HARD_D, HARD_N1, HARD_NQ, HARD_K)[0] == 2
        assert describe_dispatch(cvt_amd, metric, HARD_D, HARD_N, HARD_NQ, HARD_K)[0] == 2
        assert describe_dispatch(cvt_amd, metric, HARD_D, 32767, HARD_NQ, HARD_K)[0] != 2
        assert describe_dispatch(cvt_amd, metric, HARD_D, HARD_N, 15, HARD_K)[0] != 2


@gpu
@pytest.mark.parametrize("metric", [IP, L2F])
@pytest.mark.parametrize("rows_copy", [4, 0])
def test_predicated_rerun(amd, metric, rows_copy):
    """The threshold filter on the smallest table it takes, built by two appends with an odd seam and searched after each: the filter
    answers what its bound covers and flags the rest, flat_f32_sq_kernel re-runs under the flags (flat_skip: a group with one flagged query
    of four, groups with none, a group with four, a group with clamped padding queries) and the merge overwrites the flagged queries
    alone (measured: 7 of the 18 queries flagged under IP, 5 under L2F, after either append).  With the row-major copy
    ("flat_f32_rows_copy" 4) flat_unblock_kernel first copies every block, then only from block 512 on"""
    n1, n, D, nq, k = HARD_N1, HARD_N, HARD_D, HARD_NQ, HARD_K
    db, q, model1, model2 = hard_table(metric)
    with tuned(amd, flat_f32_rows_copy=rows_copy, **HARD_TUNE):
        ix = amd.FlatIndex(metric, D)
        try:
            for a, b, (mb, mi) in ((0, n1, model1), (n1, n, model2)):
                with amd.launch_log() as log:
                    ix.add(db[a:b])
                assert [name for name, *_ in log].count(BLOCK) == 1, log
                with amd.launch_log() as log:
                    d, i = ix.search(q, k)
                names = [name for name, *_ in log]
                ran = searched(log)
                redo = ix.last_redo()
                assert ix.last_search()[0] == 3, (ix.last_search(), names)
                assert 0 < redo < nq, redo
                assert set(ran) == {*TFILTER, SQ} and len(ran[TFILTER[0]]) == 2, ran          # the sample pass and the filter pass
                assert max(names.index(t) for t in TFILTER) < names.index(SQ) < names.index("topk_merge_kernel"), names
                splits = max(plan_splits(b, nq, 4), min(32, b // 8192))                         # flat_search_rows: a predicated run
                assert splits == 16 and ran[SQ] == [((-(-nq // 4) * splits, 1, 1), 256, 0)], ran
                unblock = [(g, bl) for name, g, bl, _ in log if name == UNBLOCK]
                assert unblock == ([((-(-b // 64) - a // 64, 1, 1), 256)] if rows_copy else []), (unblock, a // 64)
                bits = np.ascontiguousarray(d).view(np.uint32)
                bad = np.flatnonzero(np.any(i != mi, axis=1) | np.any(bits != mb, axis=1))
                assert bad.size == 0, (b, "queries", bad.tolist(), i[bad[:1]].tolist(), mi[bad[:1]].tolist(), bits[bad[:1]].tolist(), mb[bad[:1]].tolist())
        finally:
            ix.close()


# ---- 7. non-finite input ----

@gpu
@pytest.mark.parametrize("metric", [IP, L2F])
@pytest.mark.parametrize("D", [32, 5])
@pytest.mark.parametrize("n", [200, 4500])
def test_non_finite_input(amd, metric, D, n):
    """A row with a +NaN element, a row with +inf, a row of -inf; a query holding NaN and one holding +inf (in the +inf row's column: inf - inf).
    The rule of cvtmi_flat_search_masked / cvtmi_flat_rerank: a NaN distance is a real candidate, ordered by its key.  The model's NaNs
    say WHICH (query, row) pairs are NaN, not where they rank: the device's subtractions (q - x, 1 - sum) negate an operand, so a NaN that
    went through one carries the sign bit on the MI355X and its key is below -inf's -- measured: every NaN distance comes back as
    0xffc00000 and, for a finite query, leads the list; only the NaN query under L2F (the NaN is the first operand of q - x) returns
    0x7fc00000.  Each list is therefore judged by the keys of the bits it returns: sign-bit NaNs, then the model's ranking of the non-NaN rows
    (a +inf distance is one of them), then NaNs without a sign bit, and those only once every non-NaN row is listed.
    200 rows: one split, k up to every non-NaN row; 4500 rows: two splits and the merge"""
    nq = 5
    db, q = table(700 + n + D + metric, metric, n, D, nq)
    db[13, D // 3] = np.nan; db[14, D // 4] = np.inf; db[15] = -np.inf
    q[2, 1] = np.nan; q[3, D // 4] = np.inf
    dist = distances(metric, db, q)
    nan_m = np.isnan(dist)
    finite_q = [0, 1, 4]
    assert nan_m[2].all() and all(nan_m[j, 13] and not nan_m[j].all() for j in (0, 1, 3, 4))
    m_min = int(min((~nan_m[j]).sum() for j in finite_q))
    assert n - 3 <= m_min < n                                   # (finite queries: k below is at most the count of non-NaN rows)
    for k in (10, min(m_min, 2048)):
        d, i, ran, last = search(amd, metric, db, q, k, seam=odd_seam(n))
        expect_exact(ran, last, n, D, nq, k)
        b = np.ascontiguousarray(d).view(np.uint32)
        for j in range(nq):
            what = (metric, D, n, k, j, i[j, :12].tolist(), [hex(v) for v in b[j, :12]])
            valid = i[j] >= 0
            rows = i[j][valid]
            got = b[j][valid]
            assert rows.size == min(k, n) and valid[:rows.size].all() and np.all(b[j][~valid] == PAD), what
            assert np.unique(rows).size == rows.size and rows.max() < n, what                                    # distinct rows
            key = (f32_key(got).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
            assert np.all(key[1:] > key[:-1]), what                                                             # ascending (key of the returned bits, row)
            got_nan = np.isnan(got.view(np.float32))
            assert np.array_equal(got_nan, nan_m[j, rows]), what                                                # NaN exactly where the model's is
            assert np.array_equal(got[~got_nan], dist[j].view(np.uint32)[rows[~got_nan]]), what                 # the model's bits elsewhere
            m = int((~nan_m[j]).sum())
            if m == 0:                                                                                         # the NaN query
                assert got_nan.all(), what
                continue
            order = ranking(np.where(nan_m[j], np.float32(np.inf), dist[j]))
            order = order[~nan_m[j][order]]                                                                    # the model's ranking of the non-NaN rows
            c = int((~got_nan).sum())
            assert np.array_equal(rows[~got_nan], order[:c]), (what, c, m, order[:12].tolist())
            unsigned_nan = got_nan & (got < 0x80000000)
            assert c == m or (not unsigned_nan.any() and c + int(got_nan.sum()) == k), (what, c, m)            # +inf ranks before an unsigned NaN
            assert c >= min(k, m) - (n - m), (what, c, m)                                                      # at most every NaN row ahead of them
        if k > 10 and n == 200 and metric == L2F:
            assert np.any(b[finite_q] == PAD)                   # +inf distances with a label made it into the lists
