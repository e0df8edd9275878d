"""GPU parity of the fp32 stream (flat_f32_stream.hip, route 2) across its group and pass geometry.

The stream splits each row stream's tiles into NG groups of G <= 32 tiles (fs_groups); a group entry keeps the (best, second) key of
one lane, the key's low five bits carry the tile's place in the group, and the collect / finish kernels turn an entry back into a row
from (group, stream, lane, place).  Every case here names the (G, NG) it targets for each form of the stream kernel (checked against a
restatement of fs_groups), plants the queries' nearest rows where that decoding can go wrong -- two and three tiles of one group, the
last tile of a group and the first of the next, the stream's last (ragged) group, the table's last partial tile, exact duplicates --
and compares lists and distance bits on every query with the exact kernels (flat_variant 1), on a sample that holds every planted
query with the checker.  Every case also asserts route 2 and how many queries the exact kernels re-answered (flat_count_redo), so
that no case can pass because the stream gave up."""
import numpy as np
import pytest

from conftest import bits
from test_gpu_flat_f32_bounds import _band_check, _near_tie_table, _oracle, _same

pytestmark = pytest.mark.gpu
IP, L2F = 0, 1
FS_WAVES, FSS_STREAMS = 1024, 256      # row streams of the private-ring and the shared-ring kernels
# form -> tuning ("flat_f32_share", "flat_f32_packed") and row streams
FORMS = {"private": (0, 0, FS_WAVES), "packed": (0, 1, FS_WAVES), "share4": (1, 0, FSS_STREAMS)}


def fs_groups(n, streams):
    """tiles per group and groups per row stream (flat_f32_stream.hip, fs_groups)"""
    n_tiles = -(-n // 32)
    per = -(-n_tiles // streams)
    g = 32
    while g > 1 and g // 2 >= per:
        g //= 2
    return g, -(-per // g)


def fs_qb_max(D):
    """query blocks of 32 a wave holds (flat_f32_stream.hip, fs_qb_max)"""
    qb = 4
    while qb > 1 and qb * (8 * (D // 16) + 48) > 368:
        qb -= 1
    return qb


def _pass_size(D, nq):
    """queries per pass of a batch (api_flat.hip, flat_search_streamed; the four-wave shared ring at D / 16 % 4 == 0)"""
    qpriv = 32 * fs_qb_max(D)
    qmax = 4 * qpriv if (D // 16) % 4 == 0 else qpriv
    passes = -(-nq // qmax)
    if qpriv < nq <= 2 * qpriv:
        passes = 2
    return -(-nq // passes)


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()
    cvt_amd.set_tuning("flat_count_redo", 1)
    yield cvt_amd
    cvt_amd.set_tuning("flat_count_redo", 0)


def _tunings(amd, share=0, packed=1, min_rows=262144):
    amd.set_tuning("flat_f32_tfilter", 0); amd.set_tuning("flat_f32_stream", 2)
    amd.set_tuning("flat_f32_share", share); amd.set_tuning("flat_f32_packed", packed)
    amd.set_tuning("flat_f32_tfilter_min_rows", min_rows)


def _restore(amd):
    amd.set_tuning("flat_variant", 0); amd.set_tuning("flat_f32_tfilter", 4); amd.set_tuning("flat_f32_stream", 1)
    amd.set_tuning("flat_f32_share", 0); amd.set_tuning("flat_f32_packed", 1); amd.set_tuning("flat_f32_tfilter_min_rows", 262144)


def _stream_rows(n, streams, G, NG, s, lane):
    """rows of row stream s, lane `lane`, at the tile places that exercise the groups: (two tiles of group 0, three tiles of group g,
    the last tile of group g and the first of group g + 1, the stream's last tile)"""
    n_tiles = -(-n // 32)
    my = -(-(n_tiles - s) // streams)
    g = max(0, NG - 2)
    places = [1, 2, g * G, g * G + G // 2, g * G + G - 1, (g + 1) * G, my - 1]
    out = []
    for i in places:
        r = (s + i * streams) * 32 + lane
        if 0 <= i < my and r < n and r not in out:
            out.append(r)
    return out


def _table(metric, D, n, nq, seed, planted):
    """unit-norm clustered rows and queries (generated on the GPU); query j in `planted` owns rows at the places of _stream_rows in
    both stream counts (1024 and 256), at distances 1e-3 ... 1e-2 from it (near ties for the stream, distinct for the exact
    distances), plus an exact duplicate of its nearest planted row one group further on; the first planted query also owns the
    table's last two rows (its last, partial tile)"""
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(seed)
    cen = torch.randn((300, D), generator=g, device=dev)
    x = cen[torch.randint(0, 300, (n,), generator=g, device=dev)] + 0.5 * torch.randn((n, D), generator=g, device=dev)
    x = x / x.norm(dim=1, keepdim=True)
    q = x[torch.randint(0, n, (nq,), generator=g, device=dev)] + 0.2 * torch.randn((nq, D), generator=g, device=dev)
    q = q / q.norm(dim=1, keepdim=True)
    used = set()
    for c, j in enumerate(planted):
        rows = []
        for streams in (FS_WAVES, FSS_STREAMS):
            G, NG = fs_groups(n, streams)
            rows += _stream_rows(n, streams, G, NG, (97 * c + 13 * streams // 256 + 5) % streams, (7 * c + 3) % 32)
        if c == 0:
            rows += [n - 1, n - 2]
        rows = [r for r in dict.fromkeys(rows) if r not in used]
        used.update(rows)
        eps = torch.linspace(1e-3, 1e-2, len(rows), device=dev)
        u = torch.randn((len(rows), D), generator=g, device=dev)
        x[torch.tensor(rows, device=dev)] = q[j][None, :] + eps[:, None] * u / u.norm(dim=1, keepdim=True)
        # an exact duplicate of the nearest one, G tiles further on in its stream (ties broken by the row number)
        G, _ = fs_groups(n, FSS_STREAMS)
        dup = rows[0] + G * FSS_STREAMS * 32
        if dup < n and dup not in used:
            x[dup] = x[rows[0]]
            used.add(dup)
    return x.contiguous(), q.contiguous()


def _check_sample(orc, metric, x_np, q, ds, is_, k, sample):
    od, oi = _oracle(orc, metric, x_np, q[sample].cpu().numpy(), k)
    _same(ds[sample], is_[sample], od, oi, "checker")


def _run_forms(amd, orc, metric, D, n, forms, planted, ks=(100,), seed=0):
    """one table, every (form, (G, NG), batch sizes) of `forms` against the exact kernels and the checker"""
    import torch
    nq = max(max(b) for _, _, b in forms)
    x, q = _table(metric, D, n, nq, seed or n + D + metric, [j for j in planted if j < nq])
    try:
        ix = amd.FlatIndex(metric, D); ix.add(x)
        amd.set_tuning("flat_variant", 1)
        de, ie = ix.search(q, max(ks))
        torch.cuda.synchronize()
        assert ix.last_search()[0] == 0
        de = de.cpu().numpy(); ie = ie.cpu().numpy()
        amd.set_tuning("flat_variant", 0)
        x_np = x.cpu().numpy()
        for form, geom, batches in forms:
            share, packed, streams = FORMS[form]
            assert fs_groups(n, streams) == geom, (form, fs_groups(n, streams), geom)
            _tunings(amd, share=share, packed=packed, min_rows=32768 if packed else 262144)
            for b in batches:
                # the form the batch's passes reach: the private rings up to 32 fs_qb_max queries, the shared ring beyond
                assert (_pass_size(D, b) > 32 * fs_qb_max(D)) == (streams == FSS_STREAMS), (form, b)
                for k in ks:
                    ds, is_ = ix.search(q[:b], k)
                    torch.cuda.synchronize()
                    what = "%s G=%d NG=%d nq=%d k=%d" % (form, geom[0], geom[1], b, k)
                    assert ix.last_search()[0] == 2, what
                    assert ix.last_redo() == 0, (what, ix.last_redo())
                    ds = ds.cpu().numpy(); is_ = is_.cpu().numpy()
                    _same(ds, is_, de[:b, :k], ie[:b, :k], what)
            sample = sorted(set(j for j in planted if j < b) | {b - 1})
            _check_sample(orc, metric, x_np, q, ds, is_, ks[-1], sample)
        ix.close()
    finally:
        _restore(amd)


PLANTED = [0, 1, 31, 32, 63, 95, 127, 128, 200, 255, 256, 300, 383, 384, 450, 499, 511]


@pytest.mark.parametrize("metric,D,n,forms", [
    # private ring: G = 4 < 32; shared ring: G = 16, one group
    (L2F, 64, 100_003, [("private", (4, 1), (1, 70)), ("share4", (16, 1), (260, 300, 512))]),
    # private ring and its operand-copy form: G = 16, one group (QB 1 ... 4 / 1 ... 3); shared ring (QB 3, 3, 4, 4): G = 32, two groups, the second
    # of 5 tiles, ragged last tile
    (IP, 64, 300_013, [("private", (16, 1), (1, 40, 70, 128)), ("packed", (16, 1), (1, 40, 96)), ("share4", (32, 2), (257, 300, 400, 512))]),
    # 128-d: private ring G = 8; shared ring (QB 1 ... 3) G = 32 exactly, one group
    (IP, 128, 250_001, [("private", (8, 1), (1, 96)), ("share4", (32, 1), (193, 300, 384))]),
    # private ring and operand copy G = 32 exactly, one group; shared ring four groups
    (L2F, 64, 1_000_003, [("private", (32, 1), (1, 33, 96, 128)), ("packed", (32, 1), (1, 40, 96)), ("share4", (32, 4), (300,))]),
    # private ring and operand copy, two groups: the second of 2 tiles, ragged last tile (32-d: QB 1 ... 4)
    (L2F, 32, 1_100_007, [("private", (32, 2), (1, 40, 70, 128)), ("packed", (32, 2), (1, 96))]),
    (IP, 64, 1_100_007, [("private", (32, 2), (1, 128)), ("packed", (32, 2), (40, 96))]),
    # shared ring, eight groups, the last of 8 tiles
    (L2F, 64, 1_900_013, [("share4", (32, 8), (260, 512))]),
])
def test_stream_group_geometry(amd, orc, metric, D, n, forms):
    """each form of the stream kernel at the (G, NG) listed with it: one group narrower than 32 tiles, one group of exactly 32 (all five
    place bits), two groups with a ragged last group and last tile, eight groups; the rows planted for the first query blocks
    (PLANTED) put best and second of one group, three answers in one group, answers on both sides of a group boundary, in the
    stream's last tile, in the table's last partial tile and exact duplicates across groups into each query's top 100"""
    _run_forms(amd, orc, metric, D, n, forms, PLANTED, ks=(6, 100))


@pytest.mark.parametrize("metric,D,n,geom,per", [
    (L2F, 64, 300_007, (32, 2), 500),     # shared ring, four waves of 128 queries: two passes of 500
    (IP, 128, 300_007, (32, 2), 334),     # 128-d: 384 queries a pass, three passes of 334 (the last 332)
    (L2F, 64, 1_000_003, (32, 4), 500),
])
def test_stream_pass_geometry(amd, orc, metric, D, n, geom, per):
    """1000 queries on the shared ring in passes of `per` (api_flat.hip: per = ceil(nq / passes)), rows planted for queries in the first and
    last wave of every pass and in its partial last wave; and just under twice a private-ring pass (two passes of the private ring,
    G and NG as fs_groups gives for 1024 streams).  The later passes write their redo flags and list counters at offset a: no query
    may be re-answered, every list must equal the exact kernels'"""
    nq, qpriv = 1000, 32 * fs_qb_max(D)
    assert _pass_size(D, nq) == per and fs_groups(n, FSS_STREAMS) == geom
    bp = 2 * qpriv - 10
    assert _pass_size(D, bp) == qpriv - 5
    planted = sorted({0, 127, 128, 333, 334, 383, 384, 447, 448, 470, 499, 500, 627, 640, 664, 667, 668, 883, 884, 947, 970, 999,
                      qpriv - 6, qpriv - 5, bp - 1})
    _run_forms(amd, orc, metric, D, n, [("share4", geom, (nq,)), ("private", fs_groups(n, FS_WAVES), (bp,))], planted)


def test_stream_reproducer_2m_rows(amd, orc):
    """the shape that made the eight- and twelve-wave shared rings drop a query's rank-99 row (tools/f32_tfilter_widths.py with DS=64
    GB=0.5): 2 097 152 unit-norm 64-d rows generated from a generator seeded with 64, L2, k = 100, its 1000-query draw (after its 64- and
    128-query draws); G = 32, NG = 8 on the shared ring, no ragged group.  The four-wave form (passes of 500) and the default choice
    must equal the exact kernels; the removed forms ("flat_f32_share" 2 and 3) are refused"""
    import torch
    dev = torch.device("cuda", 0)
    D, k, nq = 64, 100, 1000
    n = int(0.5 * 2 ** 30 / (4 * D))
    assert n == 2_097_152 and fs_groups(n, FSS_STREAMS) == (32, 8)
    g = torch.Generator(device=dev); g.manual_seed(D)
    cen = torch.randn((3000, D), generator=g, device=dev)
    x = cen[torch.randint(0, 3000, (n,), generator=g, device=dev)] + 0.6 * torch.randn((n, D), generator=g, device=dev)
    x = x / x.norm(dim=1, keepdim=True)
    for m in (64, 128, nq):
        q = x[torch.randint(0, n, (m,), generator=g, device=dev)] + 0.2 * torch.randn((m, D), generator=g, device=dev)
        q = (q / q.norm(dim=1, keepdim=True)).contiguous()
    try:
        for bad in (2, 3):
            with pytest.raises(RuntimeError):
                amd.set_tuning("flat_f32_share", bad)
        ix = amd.FlatIndex(L2F, D); ix.add(x)
        amd.set_tuning("flat_variant", 1)
        de, ie = ix.search(q, k)
        torch.cuda.synchronize()
        de = de.cpu().numpy(); ie = ie.cpu().numpy()
        amd.set_tuning("flat_variant", 0)
        for share in (0, 1):
            _tunings(amd, share=share)
            ds, is_ = ix.search(q, k)
            torch.cuda.synchronize()
            assert ix.last_search()[0] == 2 and ix.last_redo() == 0, (share, ix.last_redo())
            _same(ds.cpu().numpy(), is_.cpu().numpy(), de, ie, "share %d" % share)
        ix.close()
    finally:
        _restore(amd)
    od, oi = _oracle(orc, L2F, x.cpu().numpy(), q[[0, 333, 499, 500, 999]].cpu().numpy(), k)
    _same(de[[0, 333, 499, 500, 999]], ie[[0, 333, 499, 500, 999]], od, oi, "exact kernels")


@pytest.mark.parametrize("form,D,n1,n2,nq1,nq2", [
    ("share4", 64, 524_288, 532_283, 500, 300),      # 16 384 tiles (two full groups per stream), then 16 634: streams 250 ... 255 lack group 2
    ("private", 32, 1_048_576, 1_080_000, 128, 64),  # 32 768 tiles (one full group), then 33 750: streams 982 ... 1023 lack group 1
])
def test_stream_absent_groups(amd, orc, form, D, n1, n2, nq1, nq2):
    """NG is the group count of the LONGEST stream; a shorter stream has no tile, and writes no entry, in its last group.  The
    scratch those entries occupy still holds what an earlier search left there (here: a search over a table of whole groups whose
    queries are rows, keys near their maximum); the search after the append -- queries far from every row -- must not take them
    for groups of its own"""
    import torch
    share, packed, streams = FORMS[form]
    G, NG1 = fs_groups(n1, streams)
    assert (G, NG1) == (32, n1 // (32 * 32 * streams))                 # every stream: NG1 whole groups
    G2, NG2 = fs_groups(n2, streams)
    assert (G2, NG2) == (32, NG1 + 1) and -(-n2 // 32) < streams * 32 * NG1 + streams   # some streams: no tile in group NG1
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(n2)
    c = torch.randn((D,), generator=g, device=dev)
    c = c / c.norm()
    x = torch.randn((n2, D), generator=g, device=dev)
    x[:n1] = c[None, :] + 0.1 * x[:n1] / D ** 0.5          # the first table: one tight cluster around c
    x = x / x.norm(dim=1, keepdim=True)
    q1 = x[torch.randint(0, n1, (nq1,), generator=g, device=dev)].contiguous()
    q2 = -c[None, :] + 0.3 * torch.randn((nq2, D), generator=g, device=dev) / D ** 0.5
    q2 = (q2 / q2.norm(dim=1, keepdim=True)).contiguous()   # far from the cluster: the appended rows hold its neighbours
    k = 100
    try:
        _tunings(amd, share=share, packed=packed)
        ix = amd.FlatIndex(L2F, D); ix.add(x[:n1])
        ix.search(q1, k)                                   # (fills the scratch with keys near the maximum: what the lists hold is not the point)
        assert ix.last_search()[0] == 2
        ix.add(x[n1:])
        ds, is_ = ix.search(q2, k)
        torch.cuda.synchronize()
        assert ix.last_search()[0] == 2
        assert ix.last_redo() == 0, ix.last_redo()
        amd.set_tuning("flat_variant", 1)
        de, ie = ix.search(q2, k)
        torch.cuda.synchronize()
        ix.close()
    finally:
        _restore(amd)
    _same(ds.cpu().numpy(), is_.cpu().numpy(), de.cpu().numpy(), ie.cpu().numpy(), form)
    _check_sample(orc, L2F, x.cpu().numpy(), q2, ds.cpu().numpy(), is_.cpu().numpy(), k, [0, nq2 - 1])


@pytest.mark.parametrize("metric,D,n,nq,form,geom,scale", [
    (L2F, 32, 1_100_007, 64, "private", (32, 2), 1.0),
    (IP, 96, 1_050_007, 48, "private", (32, 2), 1.0),     # the second group of one tile
    (L2F, 192, 300_007, 130, "share4", (32, 2), 1.0),
    (IP, 256, 300_007, 130, "share4", (32, 2), 1.0),      # margin 2^-12 Q from 129-d on
    (L2F, 256, 300_007, 130, "share4", (32, 2), 1.0),
    (L2F, 64, 1_100_007, 32, "packed", (32, 2), 1.0),     # the operand copy: margin + 2 W_q
    (IP, 64, 300_007, 260, "share4", (32, 2), 8.0),       # |theta| ~ 2^8 larger: the (2 + |theta|) 2^-20 term of the inner product
])
def test_stream_bound_edges(amd, orc, metric, D, n, nq, form, geom, scale):
    """the near-tie table of test_gpu_flat_f32_bounds.py (rows tied to within the margin around each query's k-th score) at the widths
    and forms test_stream_near_ties leaves out, on multi-group tables: a margin too small at its width drops a true neighbour"""
    rng = np.random.default_rng(D * 7 + metric + int(scale))
    ks = (1, 10, 100)
    x, q = _near_tie_table(rng, metric, n, D, nq, 160)
    if scale != 1.0:
        x *= np.float32(scale); q *= np.float32(scale)
    _band_check(metric, x, q, ks)
    share, packed, streams = FORMS[form]
    assert fs_groups(n, streams) == geom
    assert (_pass_size(D, nq) > 32 * fs_qb_max(D)) == (streams == FSS_STREAMS)
    od, oi = _oracle(orc, metric, x, q, max(ks))
    try:
        _tunings(amd, share=share, packed=packed, min_rows=32768 if packed else 262144)
        ix = amd.FlatIndex(metric, D); ix.add(x)
        for k in ks:
            ds, is_ = ix.search(q, k)
            assert ix.last_search()[0] == 2, k
            assert ix.last_redo() == 0, (k, ix.last_redo())
            _same(ds, is_, od[:, :k], oi[:, :k], "k=%d" % k)
        ix.close()
    finally:
        _restore(amd)


def test_stream_overflow_paths(amd):
    """the two lists that can run over, with exact counts of the queries handed to the exact kernels: query 1's 2200 exact duplicates
    are entries 0 ... 2199, all inside the first of three collect slices (more than its 2048 hits); query 2's 2500 duplicates are
    every third entry of group 1, under 2048 per slice but more than the 2048 a query's list holds.  The other 298 queries, which
    point away from both duplicated rows, stay"""
    rng = np.random.default_rng(11)
    D, n, nq, k = 64, 300_007, 300, 10
    assert fs_groups(n, FSS_STREAMS) == (32, 2)
    x = rng.normal(size=(n, D)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    va, vb = x[5].copy(), x[7].copy()
    x[:2200] = va                               # tiles 0 ... 68, place 0: entries (g 0, stream t, lane j) = row
    rb = 32 * 256 * 32 + 3 * np.arange(2500)    # group 1, place 0: entry 8192 + 3 m
    x[rb] = vb
    q = x[rng.integers(0, n, nq)] + 0.1 * rng.normal(size=(nq, D))
    for v in (va, vb):                          # the other queries point away from both duplicated rows: no list of theirs holds them
        q -= np.outer(q @ v, v)
    q = (q - 0.3 * (va + vb)).astype(np.float32)
    q[1] = va; q[2] = vb
    q = np.ascontiguousarray(q)
    try:
        _tunings(amd, share=1)
        ix = amd.FlatIndex(L2F, D); ix.add(x)
        ds, is_ = ix.search(q, k)
        assert ix.last_search()[0] == 2
        assert ix.last_redo() == 2, ix.last_redo()
        amd.set_tuning("flat_variant", 1)
        de, ie = ix.search(q, k)
        ix.close()
    finally:
        _restore(amd)
    assert np.array_equal(is_, ie) and np.array_equal(bits(ds), bits(de))
    assert np.array_equal(is_[1], np.arange(k)) and np.array_equal(is_[2], rb[:k])
