"""GPU: cvtmi_opq_query_video on each of its four coarse-probe routes (launch_coarse_probe, csrc/query_video.hip):

    split   coarse_probe_split_kernel + coarse_probe_merge_kernel   variant 0, coarseK >= 1024, nq < 256, nprobe <= 128
    filter  probe_score_kernel + probe_select_kernel (assign_mfma)  variant 0 with nq >= 256, or variant 2; 32 <= D <= 128,
                                                                    D % 16 == 0, coarseK >= 256, nprobe <= 48
    tile    coarse_probe_tile_kernel                                nq >= 64, nprobe <= 128, D <= 256
    single  coarse_probe_kernel                                     everything else; nprobe > 128 is refused

at the shapes and data where they can go wrong: ties at the nprobe-th list across every block boundary, the filter's
exact fallbacks and its chunk loop, split ranges with a short last part, lists of more than one 4096-entry piece,
widths other than 128, score clamps and non-finite frames.  The checker is the oracle's QueryThrehold
(orc_query_video) and, for the non-finite frames, also the reference itself where oracle/_ref is built.

The data are built so that a wrong probe list shows in the scores: every list holds its own video (video id = list id,
img_num = coarseK), and the lists a frame should probe lie close around it (every entry scores below 1.0) while all
others lie far away.  So `match_score[f] < 1.0` is exactly the probed set, and it is checked against the set the data
were designed to give, besides the oracle's bits."""
import numpy as np
import pytest

from conftest import bits

from oracle import binding as ob

pytestmark = pytest.mark.gpu

K_BLOCK = 256
PROBE_SPLITS_MAX = 64


@pytest.fixture(scope="module")
def amd():
    import torch
    torch.cuda.is_available()
    import cvt_amd
    return cvt_amd


# ---- the dispatch rule of launch_coarse_probe, as written there ----
def route_of(variant, nq, coarseK, D, nprobe):
    nprobe = min(nprobe, coarseK)                      # the API clamps first (opq_query_video_leased)
    scratch = nq < 256 and nq * PROBE_SPLITS_MAX * nprobe * 8 <= (64 << 20)
    if variant == 0 and coarseK >= 1024 and nq > 0 and scratch and 1 <= nprobe <= 128:
        return "split"
    nq_f = max(nq, 256) if variant == 2 else nq
    if variant != 1 and 32 <= D <= 128 and D % 16 == 0 and coarseK >= 256 and nq_f >= 256 and nprobe <= 48:
        return "filter"
    if nq >= 64 and nprobe <= 128 and D <= 256:
        return "tile"
    if nprobe > 128:
        return "refused"
    return "single"


VARIANT = {"split": 0, "filter": 2, "tile": 1, "single": 1}


def split_chunk(coarseK):
    splits = min((coarseK + K_BLOCK - 1) // K_BLOCK, PROBE_SPLITS_MAX)
    return ((coarseK + splits - 1) // splits + K_BLOCK - 1) // K_BLOCK * K_BLOCK


def boundaries(route, coarseK):
    """Block boundaries of the route's kernels: split ranges and their 256-centroid tiles, 64-centroid tiles (tile
    kernel), 32-centroid tiles and 1024-centroid theta tiles (filter), 256-centroid tiles (single)."""
    step = {"split": [split_chunk(coarseK), K_BLOCK], "filter": [32, 1024, K_BLOCK], "tile": [64], "single": [K_BLOCK]}[route]
    out = sorted({b for s in step for b in range(s, coarseK, s)})
    return out or [coarseK // 2]


def chain(q, c):
    """The reference's distance (IVFOPQ.cpp:244-248): d ascending, fp32, separate multiply and add.  q [D], c [n][D]."""
    acc = np.zeros(c.shape[0], np.float32)
    for d in range(c.shape[1]):
        t = np.float32(q[d]) - c[:, d]
        acc = acc + t * t
    return acc


def same_scores(a, b):
    """Bits on cells that are not NaN, NaN-ness (not the payload) on the others."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(np.where(na, 0, a)), bits(np.where(nb, 0, b)))


def _grid(x, g):
    return (np.round(np.asarray(x, np.float64) / g) * g).astype(np.float32)


class Design:
    """coarseK lists and nq frames.  Frame f sits at the anchor of region f % R.  Each region owns nprobe + 2 centroids
    close around its anchor at growing distances, with a tie at ranks nprobe - 1 / nprobe: a pair of centroids placed on
    the two sides of a block boundary of the route (the lower id must be probed).  The pair is one of
      dup   two identical centroids (or `copies` of them),
      ulp   two centroids one ulp apart in one coordinate,
      mid   p + e and p - e: the frame is their midpoint (exactly, on a power-of-two grid),
      on    two identical centroids ON the frame (ranks 0 and 1).
    The other centroids lie far away (scale-sized, like the anchors).  Every list holds `per_list` entries of video
    = list id; residuals and codebooks are small, so a probed list's entries score below 1.0."""

    def __init__(self, route, D, M, coarseK, nq, nprobe, seed, Kpq=256, scale=1.0, copies=2, per_list=2):
        rng = np.random.default_rng(seed)
        self.D, self.M, self.coarseK, self.nq = D, M, coarseK, nq
        self.nprobe = nk = min(nprobe, coarseK)
        g = scale * 2.0 ** -12 if scale <= 1 else scale * 2.0 ** -21       # anchors and offsets on one grid: p +- e exact
        ds = min(scale, 1.0)
        per = nk + copies                                                    # centroids a region owns
        R = max(1, min(nq, coarseK // per))
        coarse = _grid(rng.normal(size=(coarseK, D)) * scale, g)             # far centroids
        anchors = _grid(rng.normal(size=(R, D)) * scale, g)
        free = np.ones(coarseK, bool)

        def take(n):                                                         # n random free slots
            out = np.zeros(0, np.int64)
            while out.size < n:
                c = rng.integers(0, coarseK, size=4 * n + 16)
                c = c[free[c]]
                out = np.unique(np.concatenate([out, c]))
                out = out[rng.permutation(out.size)][:n] if out.size > n else out
            free[out] = False
            return out

        def nearest_free(i, step, n):
            out = []
            while 0 <= i < coarseK and len(out) < n:
                if free[i]: out.append(i)
                i += step
            return out
        bnds = boundaries(route, coarseK)
        kinds = ["dup", "ulp", "mid", "on"]
        self.expect, self.kind, self.pairs = [], [], []
        for r in range(R):
            kind = kinds[r % 4]
            b = bnds[(r * 7) % len(bnds)]
            # pair indices: both sides of boundary b, the nearest free slots
            lo, hi = nearest_free(b - 1, -1, 1), nearest_free(b, 1, copies - 1)
            if not lo or len(hi) < copies - 1:
                pair = sorted(take(copies).tolist())
            else:
                pair = lo + hi
            free[pair] = False
            rest = take(min(per - copies, int(free.sum())))
            p = anchors[r]
            rad = ds * (0.05 + 0.3 * (np.arange(nk + 1) + 1) / (nk + 2))      # level k: distance ~ rad[k]
            dirs = rng.normal(size=(nk + 1, D))
            dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
            delta = _grid(dirs * rad[:, None], g)
            tie = 0 if kind == "on" else nk - 1
            singles = [k for k in range(nk + 1) if k != tie]
            for idx, k in zip(rest, singles):
                coarse[idx] = p + delta[k]
            if kind == "on":
                for i in pair: coarse[i] = p
            elif kind == "mid":
                coarse[pair[0]] = p + delta[tie]
                for i in pair[1:]: coarse[i] = p - delta[tie]
            else:
                for i in pair: coarse[i] = p + delta[tie]
                if kind == "ulp":
                    j = int(rng.integers(0, D))
                    coarse[pair[-1], j] = np.nextafter(coarse[pair[-1], j], np.float32(np.inf if r % 8 < 4 else -np.inf))
            own = np.array(sorted(list(pair) + list(rest)))
            d = chain(p, coarse[own])
            order = np.lexsort((own, d))                                      # (distance, list) ascending
            self.expect.append(set(own[order[:nk]].tolist()))
            self.kind.append(kind)
            self.pairs.append(pair)
        self.R = R
        self.coarse = coarse
        self.q = anchors[np.arange(nq) % R].copy()
        self.books = (rng.normal(size=(M, Kpq, D // M)) * 0.003 * ds).astype(np.float32)
        self.lists = np.repeat(np.arange(coarseK, dtype=np.int32), per_list)
        self.videos = self.lists.copy()
        self.codes = rng.integers(0, Kpq, size=(self.lists.size, M)).astype(np.uint8)

    def index(self, amd, perm=None):
        idx = amd.OpqIndex(self.coarse, self.books, perm=perm)
        idx.add_codes(self.codes, self.lists, self.videos)
        return idx

    def csr(self):
        off = np.zeros(self.coarseK + 1, np.int64)
        np.cumsum(np.bincount(self.lists, minlength=self.coarseK), out=off[1:])
        order = np.argsort(self.lists, kind="stable")
        return off, self.codes[order], self.videos[order]

    def oracle(self, orc, q=None, nprobe=None):
        off, codes, vid = self.csr()
        q = self.q[:self.R] if q is None else q
        return orc.query_video(q, self.coarse, self.books, nprobe or self.nprobe, off, codes, vid, self.coarseK)

    def check(self, ms, oms_unique):
        """ms [nq][coarseK] against the oracle (computed on the R distinct frames) and against the designed probe sets."""
        rows = np.arange(ms.shape[0]) % self.R
        assert np.array_equal(bits(ms), bits(oms_unique[rows]))
        for f in range(ms.shape[0]):
            got = set(np.flatnonzero(ms[f] < 1.0).tolist())
            assert got == self.expect[rows[f]], (f, self.kind[rows[f]], sorted(got ^ self.expect[rows[f]]))


def run_route(amd, route, fn):
    amd.set_tuning("probe_variant", VARIANT[route])
    try:
        return fn()
    finally:
        amd.set_tuning("probe_variant", 0)


def _query(amd, route, idx, q, nprobe, img_num, device=False, rotate=False):
    import torch
    if device:
        return run_route(amd, route, lambda: idx.query_video(torch.from_numpy(q).cuda(), nprobe, img_num, rotate=rotate).cpu().numpy())
    return run_route(amd, route, lambda: idx.query_video(q, nprobe, img_num, rotate=rotate))


def _route_case(amd, orc, route, D, M, coarseK, nq, nprobe, seed, **kw):
    assert route_of(VARIANT[route], nq, coarseK, D, nprobe) == route
    des = Design(route, D, M, coarseK, nq, nprobe, seed, **kw)
    idx = des.index(amd)
    try:
        ms = _query(amd, route, idx, des.q, nprobe, coarseK, device=True)
        oms = des.oracle(orc)
        des.check(ms, oms)
        if nq <= 64:     # the host-pointer entry: the same scores
            des.check(_query(amd, route, idx, des.q, nprobe, coarseK), oms)
    finally:
        idx.close()
    return des


# ---- boundary ties on every route; split shapes (coarseK with a short last range, -1 padding in the merge) ----
SPLIT_SHAPES = [(1024, 1, 128), (1024, 255, 1), (1025, 63, 40), (1025, 64, 128), (1279, 255, 40), (1279, 1, 1),
                (16385, 64, 1), (16385, 255, 128), (20000, 63, 128), (20000, 1, 40)]


@pytest.mark.parametrize("coarseK,nq,nprobe", SPLIT_SHAPES, ids=["split-k%d-nq%d-np%d" % s for s in SPLIT_SHAPES])
def test_split_shapes_and_ties(amd, orc, coarseK, nq, nprobe):
    _route_case(amd, orc, "split", 32, 8, coarseK, nq, nprobe, seed=coarseK * 7 + nq + nprobe)


TIE_CASES = [("filter", 256, 40, 1), ("filter", 257, 300, 48), ("filter", 1007, 100, 10), ("filter", 4096, 256, 20),
             ("tile", 1000, 64, 5), ("tile", 1000, 100, 128), ("tile", 4096, 130, 49), ("tile", 257, 64, 1),
             ("single", 600, 1, 1), ("single", 600, 63, 128), ("single", 4096, 20, 40)]


@pytest.mark.parametrize("route,coarseK,nq,nprobe", TIE_CASES, ids=["%s-k%d-nq%d-np%d" % c for c in TIE_CASES])
def test_boundary_ties(amd, orc, route, coarseK, nq, nprobe):
    _route_case(amd, orc, route, 64, 8, coarseK, nq, nprobe, seed=coarseK * 5 + nq + nprobe)


# ---- widths: D % 4 != 0 (scalar branch of the split kernel), D % 16 != 0, 256 (widest tile), 320 (single only) ----
WIDTHS = {30: 6, 32: 16, 36: 4, 96: 8, 256: 16, 320: 8}
WIDTH_CASES = [(r, D) for D in WIDTHS for r in ("split", "filter", "tile", "single")
               if route_of(VARIANT[r], {"split": 70, "filter": 70, "tile": 70, "single": 9}[r], 1100, D, 12) == r]


@pytest.mark.parametrize("route,D", WIDTH_CASES, ids=["%s-d%d" % c for c in WIDTH_CASES])
def test_widths(amd, orc, route, D):
    nq = 9 if route == "single" else 70
    _route_case(amd, orc, route, D, WIDTHS[D], 1100, nq, 12, seed=D * 11 + len(route), Kpq=200 if D == 36 else 256)


def test_width_cases_cover_every_admitting_route():
    got = {(r, D) for r, D in WIDTH_CASES}
    for D in WIDTHS:
        assert ("split", D) in got and ("single", D) in got
        assert (("tile", D) in got) == (D <= 256)
        assert (("filter", D) in got) == (D % 16 == 0 and 32 <= D <= 128)


# ---- the filter's exact fallbacks ----
FALLBACKS = [("band97", "filter", dict(copies=100), 1024, 64, 10), ("np48", "filter", {}, 512, 64, 48),
             ("np49", "tile", {}, 512, 64, 49), ("q-huge", "filter", dict(scale=2.0 ** 13), 300, 64, 8),
             ("q-tiny", "filter", dict(scale=2.0 ** -34), 300, 64, 8)]


@pytest.mark.parametrize("name,route,kw,coarseK,nq,nprobe", FALLBACKS, ids=[f[0] for f in FALLBACKS])
def test_filter_fallbacks(amd, orc, name, route, kw, coarseK, nq, nprobe):
    """More than PS_CAND = 96 centroids at one distance; nprobe 48 (the filter's last) and 49 (past it: variant 2 takes the
    tile kernel); frames whose bound Q leaves (2^-60, 2^30)."""
    des = _route_case(amd, orc, route, 32, 8, coarseK, nq, nprobe, seed=1000 + [f[0] for f in FALLBACKS].index(name), **kw)
    q2 = (des.q.astype(np.float64) ** 2).sum(1) + (des.coarse.astype(np.float64) ** 2).sum(1).max()
    if name == "q-huge":
        assert q2.min() >= 2.0 ** 30
    if name == "q-tiny":
        assert q2.max() * 1.001 <= 2.0 ** -60 and np.all(np.abs(des.q[des.q != 0]) >= 2.0 ** -50)


def test_filter_chunks(amd, orc):
    """coarseK = 65 536 at D = 32: one chunk of T (512 MB) holds 2048 frames, so 4500 frames run three chunks, the last one
    ragged.  Every frame against the exact kernels (variant 1) and the designed probe set; frames from every chunk and on
    both sides of each chunk boundary against the oracle."""
    import torch
    coarseK, nq, nprobe, D = 65536, 4500, 8, 32
    assert route_of(0, nq, coarseK, D, nprobe) == "filter" and route_of(1, nq, coarseK, D, nprobe) == "tile"
    ldT = (coarseK + 31) // 32 * 32
    chunk = max(256, min(nq, (512 << 20) // (ldT * 4)))
    assert chunk == 2048 and nq % chunk and nq // chunk == 2
    des = Design("filter", D, 8, coarseK, nq, nprobe, seed=65536, per_list=1)
    assert des.R == nq
    idx = des.index(amd)
    try:
        qd = torch.from_numpy(des.q).cuda()
        a = idx.query_video(qd, nprobe, coarseK, rotate=False)                # variant 0: the filter (nq >= 256)
        b = run_route(amd, "tile", lambda: idx.query_video(qd, nprobe, coarseK, rotate=False))
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        del b
        hit = (a < 1.0).nonzero().cpu().numpy()
        assert hit.shape[0] == nq * nprobe
        got = hit[:, 1].reshape(nq, nprobe)
        for f in range(nq):
            assert set(got[f].tolist()) == des.expect[f], f
        samp = sorted({0, 1, 1000, 2046, 2047, 2048, 2049, 3000, 4094, 4095, 4096, 4097, 4499})
        oms = des.oracle(orc, q=des.q[samp])
        assert np.array_equal(bits(a[samp].cpu().numpy()), bits(oms))
        del a
    finally:
        idx.close()


# ---- lists longer than one 4096-entry piece ----
def test_long_lists(amd, orc):
    """Lists of 4096, 4097 and 3 x 4096 + 1 entries and an empty one; each video's best entry (code 0: score 0 for a frame on
    the list's centroid) sits in the last piece of its list, behind entries of the same video in earlier pieces."""
    D, M, Kpq, L = 32, 8, 64, 300
    rng = np.random.default_rng(4097)
    coarse = (rng.normal(size=(L, D))).astype(np.float32)
    books = (rng.normal(size=(M, Kpq, D // M)) * 0.02).astype(np.float32)
    books[:, 0] = 0.0
    sizes = {0: 4096, 1: 4097, 2: 3 * 4096 + 1, 3: 0}
    lists, videos, codes, best = [], [], [], {}
    for l in range(L):
        n = sizes.get(l, 1)
        v = (np.arange(n) % 40 + 1000 + 40 * l).astype(np.int32) if l in sizes else np.array([l], np.int32)
        c = rng.integers(1, Kpq, size=(n, M)).astype(np.uint8)
        if l in sizes and n:
            last = (n - 1) // 4096 * 4096                                  # first entry of the last piece
            nb = min(40, n - last)
            c[n - nb:] = 0
            v[n - nb:] = 1000 + 40 * l + np.arange(nb)
            best[l] = v[n - nb:]
        lists.append(np.full(n, l, np.int32)); videos.append(v); codes.append(c)
    lists, videos, codes = np.concatenate(lists), np.concatenate(videos), np.concatenate(codes)
    img_num = 1000 + 40 * 4
    off = np.zeros(L + 1, np.int64)
    np.cumsum(np.bincount(lists, minlength=L), out=off[1:])
    assert off[2] - off[1] == 4097 and off[3] - off[2] == 12289 and off[4] == off[3]
    idx = amd.OpqIndex(coarse, books)
    idx.add_codes(codes, lists, videos)
    q = coarse[[0, 1, 2, 3, 2, 1]].copy()
    try:
        for nprobe in (1, 4):
            for route in ("single", "tile"):
                qq = q if route == "single" else np.tile(q, (11, 1))
                assert route_of(VARIANT[route], qq.shape[0], L, D, nprobe) == route
                ms = _query(amd, route, idx, qq, nprobe, img_num, device=route == "tile")
                oms = orc.query_video(qq, coarse, books, nprobe, off, codes, videos, img_num)
                assert np.array_equal(bits(ms), bits(oms)), (nprobe, route)
            for f, l in enumerate([0, 1, 2, 3, 2, 1]):
                if l in best:
                    assert np.all(ms[f][best[l]] == 0.0)                      # the minimum came from the last piece
            if nprobe == 1:
                assert np.all(ms[3] == 1.0)                                    # a probed list that is empty
                assert np.all(ms[0][1040:] == 1.0) and (ms[0][1000:1040] < 1.0).all()
    finally:
        idx.close()


# ---- the 1.0 clamp and img_num ----
def test_score_edges(amd, orc):
    """An entry scoring exactly 1.0, entries above 1.0 (the cell stays 1.0), videos with no entry, img_num above the largest
    video id; img_num at or below it fails the call."""
    D, M, Kpq, L = 32, 4, 16, 64
    rng = np.random.default_rng(10)
    coarse = rng.normal(size=(L, D)).astype(np.float32)
    books = np.zeros((M, Kpq, D // M), np.float32)
    books[:, 1, 0] = 0.5                                                    # 4 x 0.25 = 1.0 exactly
    books[:, 2, 0] = 0.625                                                  # 4 x 0.390625 > 1.0
    books[:, 3, 0] = 0.25                                                   # 4 x 0.0625 = 0.25
    codes = np.array([[1] * M, [2] * M, [3] * M, [1] * M, [2] * M], np.uint8)
    videos = np.array([0, 1, 3, 5, 5], np.int32)                            # video 2 / 4: no entry; video 5: 1.0 and above
    lists = np.zeros(5, np.int32)
    idx = amd.OpqIndex(coarse, books)
    idx.add_codes(codes, lists, videos)
    q = np.repeat(coarse[:1], 70, axis=0)                                   # frames on centroid 0
    off = np.zeros(L + 1, np.int64); off[1:] = 5
    try:
        for route in ("single", "tile"):
            for img_num in (6, 10):
                qq = q[:9] if route == "single" else q
                ms = _query(amd, route, idx, qq, 1, img_num, device=route == "tile")
                want = np.ones(img_num, np.float32); want[3] = 0.25
                assert np.array_equal(bits(ms), bits(np.tile(want, (qq.shape[0], 1))))
                assert np.array_equal(bits(ms), bits(orc.query_video(qq, coarse, books, 1, off, codes, videos, img_num)))
            for img_num in (5, 1):
                with pytest.raises(amd.CvtmiError):
                    _query(amd, route, idx, q[:9], 1, img_num)
    finally:
        idx.close()


# ---- non-finite frames ----
NONFINITE_ROUTES = [("split", 70), ("filter", 70), ("tile", 70), ("single", 10)]


@pytest.mark.parametrize("route,nq", NONFINITE_ROUTES, ids=[r[0] for r in NONFINITE_ROUTES])
def test_nonfinite_frames(amd, orc, route, nq):
    """NaN, -NaN, a NaN whose bits are KEY_MAX (0xffffffff), +inf and 1e30 frames, through the permutation model with
    rotate=True, on the host and device entries.  A NaN frame probes lists 0 .. nprobe - 1 (every distance is NaN: the
    reference's heap keeps the first nk) and std::min leaves NaN in every video met there; +inf / 1e30 overflow every
    distance and score, and the cells stay at 1.0."""
    D, M, coarseK, nprobe = 32, 8, 1100, 12
    assert route_of(VARIANT[route], nq, coarseK, D, nprobe) == route
    des = Design(route, D, M, coarseK, nq, nprobe, seed=777 + nq)
    rng = np.random.default_rng(5)
    perm = rng.permutation(D).astype(np.int32)
    inv = np.argsort(perm)
    raw = des.q[:, inv].copy()
    special = {}
    nan = raw[1].copy(); nan[5] = np.nan; special[1] = nan
    nneg = raw[2].copy(); nneg[D - 1] = -np.nan; special[2] = nneg
    special[3] = np.full(D, np.uint32(0xffffffff)).view(np.float32).copy()
    special[4] = np.full(D, np.inf, np.float32)
    special[5] = np.full(D, 1e30, np.float32)
    kmax = raw[6].copy(); kmax[3:4] = np.array([0xffffffff], np.uint32).view(np.float32); special[6] = kmax
    for f, v in special.items():
        raw[f] = v
    assert np.signbit(raw[2, D - 1]) and np.isnan(raw[2, D - 1])
    idx = des.index(amd, perm=perm)
    try:
        off, codes, vid = des.csr()
        oms = orc.query_video(orc.reorder(perm, raw), des.coarse, des.books, nprobe, off, codes, vid, coarseK)
        met = np.zeros(coarseK, bool); met[:nprobe] = True                 # video = list id, every list holds entries
        for f in (1, 2, 3, 6):
            assert np.array_equal(np.isnan(oms[f]), met) and np.all(oms[f][~met] == 1.0)
        for f in (4, 5):
            assert np.all(oms[f] == 1.0)
        for device in (False, True):
            ms = _query(amd, route, idx, raw, nprobe, coarseK, device=device, rotate=True)
            assert same_scores(ms, oms), (route, device, [f for f in range(nq) if not same_scores(ms[f], oms[f])][:8])
        if ob.ref_available():
            # the reference itself: its own Add of one row per list (rows on the centroids), its own QueryThrehold
            rows = [des.coarse[l:l + 1][:, inv].copy() for l in range(0, coarseK, 3)]
            ref = ob.RefOPQ(des.coarse, des.books, perm)
            try:
                assert ref.index(rows) == len(rows)
                r_off, r_vid, r_codes = ref.dump()
                rms = ref.query(raw[:10], nprobe, len(rows))
            finally:
                ref.close()
            idx2 = amd.OpqIndex(des.coarse, des.books, perm=perm)
            try:
                lists = np.repeat(np.arange(coarseK, dtype=np.int32), np.diff(r_off))
                idx2.add_codes(r_codes, lists, r_vid)
                ms2 = _query(amd, route, idx2, raw[:10] if route == "single" else raw, nprobe, len(rows), rotate=True)
                assert same_scores(ms2[:10], rms)
                assert np.isnan(rms[1]).any() and np.isnan(rms[3]).any()
            finally:
                idx2.close()
    finally:
        idx.close()


# ---- nprobe: clamped above coarseK, refused above 128 ----
def test_nprobe_clamp_and_limit(amd):
    import torch
    D, M = 32, 8
    des = Design("tile", D, M, 100, 70, 100, seed=100)
    idx = des.index(amd)
    try:
        for route, nq in (("tile", 70), ("single", 9)):
            assert route_of(VARIANT[route], nq, 100, D, 105) == route
            a = _query(amd, route, idx, des.q[:nq], 105, 100)
            b = _query(amd, route, idx, des.q[:nq], 100, 100)
            assert np.array_equal(bits(a), bits(b)) and np.all(a < 1.0)   # every list probed
    finally:
        idx.close()
    des = Design("split", D, M, 1100, 300, 12, seed=101)
    idx = des.index(amd)
    try:
        for variant, nq in ((0, 10), (0, 70), (0, 300), (1, 10), (1, 70), (1, 300), (2, 10), (2, 70), (2, 300)):
            assert route_of(variant, nq, 1100, D, 129) == "refused"
            amd.set_tuning("probe_variant", variant)
            try:
                with pytest.raises(amd.CvtmiError):
                    idx.query_video(des.q[:nq], 129, 1100, rotate=False)
                with pytest.raises(amd.CvtmiError):
                    idx.query_video(torch.from_numpy(des.q[:nq]).cuda(), 129, 1100, rotate=False)
            finally:
                amd.set_tuning("probe_variant", 0)
        # 128 is taken on each of them
        for variant, nq in ((0, 10), (1, 70), (1, 10)):
            amd.set_tuning("probe_variant", variant)
            try:
                idx.query_video(des.q[:nq], 128, 1100, rotate=False)
            finally:
                amd.set_tuning("probe_variant", 0)
    finally:
        idx.close()
