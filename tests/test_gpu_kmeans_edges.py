"""k-means assignment and update on every kernel route (csrc/kmeans.hip, csrc/assign_mfma.hip, coarse_assign_kernel of
csrc/opq_encode.hip), bit for bit against the oracle (orc_pq_encode, orc_kmeans, orc_opq_train, orc_opq_learn_rotation).

Every assertion is equality with the oracle's assignments / centroid bits, or a value derived in the test's docstring.  Each test names
the route of the dispatch (launch_kmeans_assign, launch_kmeans_update, launch_coarse_assign) it is there for."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()  # raises if the HIP library is missing: there is no fallback
    return cvt_amd


def clustered(rng, n, d, k, spread=0.3):
    cen = rng.normal(size=(k, d)).astype(F32) * 3
    return (cen[rng.integers(0, k, n)] + rng.normal(size=(n, d)).astype(F32) * spread).astype(F32)


def seed_rows(n, k, seed):
    """the seeding of include/cvtmi.h: k distinct rows, index = splitmix64() % n, redraw on repeats"""
    mask = (1 << 64) - 1
    s, taken, rows = seed, set(), []
    while len(rows) < k:
        s = (s + 0x9E3779B97F4A7C15) & mask
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        z ^= z >> 31
        r = z % n
        if r not in taken:
            taken.add(r)
            rows.append(r)
    return np.array(rows, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# 1. one assignment pass against given centroids: OpqIndex(cent, books).encode(x)[0] == orc.pq_encode(x, cent, books)[0]
# ---------------------------------------------------------------------------------------------------------------------
def hard_case(rng, n, d, k, dup_at=None):
    """the recipe of test_assignment_matrix_core_filter for any n >= 1, k >= 1: a duplicate centroid (the lower index wins) and
    one a single ulp from another; rows on centroids, rows midway between two, rows scaled by 1e5 and 1e-25, an inf coordinate, a NaN
    row and a NaN in the last coordinate -- at the head of the rows and, where there is room, again at the tail (the last row sits on
    the duplicated centroid)"""
    cen = (rng.normal(size=(k, d)) * 2).astype(F32)
    if k >= 20:
        a, b, p, q = 3, 4, 7, 8
        dup_at = k // 2 if dup_at is None else dup_at
        cen[dup_at] = cen[a]
        cen[dup_at - 1] = np.nextafter(cen[b], INF)
    else:
        a, b, p, q = 0, 1 % k, 2 % k, 3 % k
        if k >= 2:
            cen[k - 1] = cen[0]
        if k >= 6:
            cen[k - 2] = np.nextafter(cen[1], INF)
    x = (cen[rng.integers(0, k, n)] + 0.4 * rng.normal(size=(n, d))).astype(F32)
    plain = (cen[rng.integers(0, k, 5)] + 0.4 * rng.normal(size=(5, d))).astype(F32)
    mid = (cen[p] + cen[q]) / F32(2)                        # equidistant up to rounding
    special = [cen[a], cen[b], mid, cen[a], mid, cen[b], plain[0] * F32(1e5), plain[1] * F32(1e-25), plain[2].copy(),
               np.full(d, np.nan, F32), plain[3].copy(), plain[4] * F32(1e5)]
    special[8][min(1, d - 1)] = np.inf
    special[10][d - 1] = np.nan
    for i, row in enumerate(special):
        if i < n:
            x[i] = row
        if n >= 3 * len(special):
            x[n - 1 - i] = row
    return cen, x


def probe(amd, orc, cen, x, variants):
    """coarse lists (and codes) of encode under every assign_variant given == the oracle's; returns the oracle's lists"""
    d = cen.shape[1]
    books = np.random.default_rng(d).normal(size=(1, 4, d)).astype(F32)   # M = 1: any d; the codes ride along
    ol, oc = orc.pq_encode(x, cen, books)
    try:
        for variant in variants:
            amd.set_tuning("assign_variant", variant)
            idx = amd.OpqIndex(cen, books)
            lists, codes = idx.encode(x)
            idx.close()
            assert np.array_equal(lists, ol), (variant, x.shape, cen.shape, np.argwhere(lists != ol)[:10].ravel())
            assert np.array_equal(codes, oc), (variant, x.shape, cen.shape)
    finally:
        amd.set_tuning("assign_variant", 0)
    assert (ol == -1).any() or x.shape[0] < 10     # the NaN row is among the first ten
    return ol


@pytest.mark.parametrize("n,d,k", [(4096, 48, 64), (4097, 48, 65), (4351, 48, 95), (4097, 48, 97), (4096, 48, 1000),
                                   (4351, 80, 64), (4096, 80, 65), (4097, 80, 95), (4351, 80, 97), (4097, 80, 1000),
                                   (4097, 112, 64), (4351, 112, 65), (4096, 112, 95), (4096, 112, 97), (4351, 112, 1000),
                                   (4097, 32, 97), (4351, 128, 65)])
def test_filter_odd_chunk_counts(amd, orc, n, d, k):
    """route: assign_filter_kernel<NCH> for NCH = 3, 5, 7 (d = 48, 80, 112: TILE is no multiple of the 512 threads, so LPT rounds up
    and fetch() clamps f < TILE), with NCH = 2 and 8 as controls; k with a ragged last tile of 32 (padding centroids); n one row and
    255 rows past a 256-row workgroup pass (clamped tail rows, a workgroup with one live wave).  variant 2 = variant 0 here (n >= 4096);
    variant 1 sends the same rows through kmeans_assign_reg_kernel<64 / 128>."""
    cen, x = hard_case(np.random.default_rng(n + d + k), n, d, k)
    probe(amd, orc, cen, x, (2, 1))


@pytest.mark.parametrize("d", [48, 80, 112])
@pytest.mark.parametrize("n", [1, 33, 255])
def test_filter_few_rows(amd, orc, n, d):
    """route: assign_filter_kernel<3 / 5 / 7> forced (variant 2) on fewer rows than one workgroup pass: n = 1 (every lane reads the
    clamped row 0), 33 (the second wave holds one live row), 255.  variant 0 at k >= 256 takes the split / fold path for the same
    rows, at k < 256 the exact kernel."""
    for k in (64, 97, 1000):
        cen, x = hard_case(np.random.default_rng(n + d + k), n, d, k)
        probe(amd, orc, cen, x, (2, 1, 0))


@pytest.mark.parametrize("n,d,k", [(4097, 40, 97), (4097, 100, 97), (4097, 48, 63), (4351, 112, 63)])
def test_filter_does_not_apply(amd, orc, n, d, k):
    """route: assign_filter_applies() == false inside 32 <= d <= 128 (d % 16 != 0) and just under k = 64: variants 0 and 2 must take
    kmeans_assign_reg_kernel<64 / 128> (a filter launched at d = 40 would read d / 16 = 2 chunks of the row) and still match"""
    cen, x = hard_case(np.random.default_rng(n + d + k), n, d, k)
    probe(amd, orc, cen, x, (2, 0, 1))


@pytest.mark.parametrize("d", [1, 8, 9, 16, 17, 33, 65, 128])
def test_exact_kernels_at_template_boundaries(amd, orc, d):
    """route: kmeans_assign_reg_kernel<DMAX> at d = DMAX and d = DMAX + 1 of every instantiation (8, 16, 32, 64, 128), k around one
    register tile of 16 centroids (1, 15, 16, 17, 33: the k bound inside the tile), n = 1, one row short of a workgroup and one past it"""
    for k in (1, 15, 16, 17, 33):
        for n in (1, 255, 257):
            cen, x = hard_case(np.random.default_rng(1000 * d + 10 * k + n), n, d, k)
            probe(amd, orc, cen, x, (1, 0))


@pytest.mark.parametrize("k,d", [(256, 8), (257, 33), (1000, 65), (8192, 9)])
def test_split_fold_path(amd, orc, k, d):
    """route: variant 0, n < 4096, k >= 256: launch_kmeans_assign_split (blockIdx.y walks csplit centroids) + kmeans_assign_fold_kernel.
    The duplicate of centroid 3 is the LAST centroid, so it lies in the last split and only the fold's strict '<' in ascending split
    order keeps index 3 for the rows that sit on it; k = 257, 1000 leave a short last split."""
    for n in (1, 300, 4095):
        cen, x = hard_case(np.random.default_rng(k + d + n), n, d, k, dup_at=k - 1)
        ol = probe(amd, orc, cen, x, (0, 1))
        assert ol[0] == 3                                   # (the oracle: the first of the two equal centroids)


@pytest.mark.parametrize("n,d,k,variants", [(300, 48, 256, (0, 1, 2)), (4100, 48, 256, (0, 1)), (300, 8, 300, (0, 1)),
                                            (300, 129, 3, (0,)), (300, 512, 33, (0,))])
def test_start_value_boundary(amd, orc, n, d, k, variants):
    """route: the start value 4294967296.0f of the argmin -- kmeans_assign_reg_kernel (variant 1), the filter's resolve of rows with
    Q >= 2^30 (variant 2; variant 0 at n = 4100), the split / fold path (variant 0, n = 300, k >= 256: both the partial minima and the
    fold start there) and coarse_assign_kernel (d > 128).
    One centroid is all zeros; every other centroid has a negative first coordinate, so for the rows below it is the only one within
    2^32.  Row 0 = (65536, 0, ...): squared distance exactly 2^32, not below the start value: -1.  Row 1 = (65536 - 2^-8, 0, ...):
    (2^16 - 2^-8)^2 = 2^32 - 2^9 + 2^-16, rounds to 2^32 - 512: assigned to the zero centroid.  Row 2 = (65536, 2^-20, 0, ...):
    2^32 + 2^-40 rounds to 2^32: -1."""
    rng = np.random.default_rng(n + d + k)
    cen = (rng.normal(size=(k, d)) * 2).astype(F32)
    cen[:, 0] = -np.abs(cen[:, 0]) - F32(1)
    z = 5 if k > 5 else 1
    cen[z] = 0
    x = (cen[rng.integers(0, k, n)] + 0.4 * rng.normal(size=(n, d))).astype(F32)
    x[:3] = 0
    x[0, 0] = 65536
    x[1, 0] = np.nextafter(F32(65536), F32(0))
    x[2, 0] = 65536
    x[2, 1] = F32(2.0 ** -20)
    x[n - 1] = x[0]
    ol = probe(amd, orc, cen, x, variants)
    assert ol[0] == -1 and ol[1] == z and ol[2] == -1 and ol[n - 1] == -1


@pytest.mark.parametrize("D", [129, 256, 257, 512])
def test_coarse_assign_wide_rows(amd, orc, D):
    """route: coarse_assign_kernel (opq_encode.hip), the D > 128 coarse assignment of encode -- cvtmi_opq_create accepts D > 128 with
    coarseK > 1.  D = one dimension past an LDS chunk of 128, exactly two chunks, one past two, and four (the k-means limit); coarseK
    under, one past and two past one LDS tile of 32 centroids; rows over more than one workgroup."""
    for coarseK in (3, 33, 70):
        cen, x = hard_case(np.random.default_rng(D + coarseK), 600, D, coarseK)
        probe(amd, orc, cen, x, (0, 1))


# ---------------------------------------------------------------------------------------------------------------------
# 2. whole k-means runs
# ---------------------------------------------------------------------------------------------------------------------
def check_kmeans(amd, orc, x, k, niter, seeds=(1, 12345), device=False):
    """amd.kmeans == orc.kmeans: iterations, assignments, centroid bits; device: also from a torch CUDA tensor.  Returns the last
    (centroids, assignments) of the oracle and of the library."""
    for seed in seeds:
        oc, oa, oit = orc.kmeans(x, k, niter, seed)
        gc, ga, git = amd.kmeans(x, k, niter, seed)
        assert git == oit, (seed, git, oit)
        assert np.array_equal(ga, oa), (seed, np.argwhere(ga != oa)[:10].ravel())
        assert np.array_equal(bits(gc), bits(oc)), (seed, np.argwhere(bits(gc) != bits(oc))[:10])
        if device:
            import torch
            tc, ta, tit = amd.kmeans(torch.from_numpy(x).cuda(), k, niter, seed)
            assert tit == oit and np.array_equal(ta.cpu().numpy(), oa) and np.array_equal(bits(tc.cpu().numpy()), bits(oc))
    return oc, oa, gc, ga


def rough_rows(rng, n, d, k):
    x = clustered(rng, n, d, max(2, k // 2))
    x[5] = x[6]                         # exact duplicate rows
    x[17] = np.nan                      # rows no centroid can claim: -1, left out of every mean and count
    x[18, d - 1] = np.inf
    return x


@pytest.mark.parametrize("n,d,k,niter,seeds,device", [(1500, 129, 17, 0, (1, 12345), True), (1200, 256, 48, 2, (1, 12345), False),
                                                      (900, 257, 5, 0, (1, 12345), False), (700, 512, 33, 2, (1, 12345), False),
                                                      (700, 450, 6, 1, (1, 12345), False), (4500, 449, 20, 2, (1, 12345), True),
                                                      (4200, 512, 512, 1, (1,), False)])
def test_kmeans_wide_rows(amd, orc, n, d, k, niter, seeds, device):
    """route: the generic kmeans_assign_kernel (d > 128): d = 129, 256 (exactly two LDS chunks), 257, 512 (the API limit), k over more
    than one 16-centroid tile; kmeans_update_kernel (n < 4096) with the last of its KM_DPL = 8 slots per lane partly used (d = 450)
    and full (512); the scatter update (n >= 4096) with 57 and 64 dimension columns, and at k = 512 its largest LDS request
    (512 * 8 * 16 + 512 * 4 bytes = 67.5 KB, above 64 KB: hipFuncSetAttribute).  The last shape is two oracle passes of 1.1e9
    operations, so it runs one seed."""
    check_kmeans(amd, orc, rough_rows(np.random.default_rng(n + d + k), n, d, k), k, niter, seeds, device)


@pytest.mark.parametrize("d", [20, 8])
def test_kmeans_update_routing(amd, orc, d):
    """route: launch_kmeans_update on both sides of both switches, same rows: n = 4095 (kmeans_update_kernel) / 4096 (scatter + proof),
    k = 512 (scatter, the 67.5 KB LDS request) / 513 (kmeans_update_kernel); d = 20 leaves a ragged last 8-dimension column of 4"""
    x = rough_rows(np.random.default_rng(d), 5000, d, 80)
    for n, k in ((4095, 64), (4096, 64), (5000, 512), (5000, 513)):
        check_kmeans(amd, orc, x[:n], k, 2, device=(n == 4096))


@pytest.mark.parametrize("n,d,k", [(5000, 8, 64), (3000, 8, 64), (4500, 48, 64)])
def test_kmeans_empty_clusters(amd, orc, n, d, k):
    """route: clusters without members -- kmeans_finalize_kernel's `m == 0` return (n >= 4096), kmeans_update_kernel's `cnt > 0`
    (n < 4096); d = 48 sends rows that all tie between duplicate centroids through the filter's resolve.  The rows are drawn from k / 4
    distinct points, so most seed rows are duplicates: the lower index takes every member and the others keep their seed."""
    rng = np.random.default_rng(n + d)
    pts = (rng.normal(size=(k // 4, d)) * 3).astype(F32)
    x = pts[rng.integers(0, k // 4, n)]
    oc, oa, gc, ga = check_kmeans(amd, orc, x, k, 2)
    assert len(np.unique(oa)) <= k // 4                     # (the oracle: at most one live cluster per distinct point)


def designed(rng, n, k, d, seed, payload):
    """rows whose cluster is chosen by the test.  Coordinates 0 and 1 place the clusters: seed row c (restated seeding) sits at centre c
    of a 32-wide grid with `gap` between centres, every other row at the centre of its chosen cluster, all with noise <= 0.1.  The
    other coordinates stay within [-2, 2] (filler: uniform [1, 2)), far too little to change an argmin: gap = 10 for d <= 16, 100
    above.  Cluster sizes are equal and even, rows left over go to cluster 0.  payload = {column: f(m, rng) -> m values}, applied
    per cluster to its rows in ascending order.  Returns (x, member)."""
    rows = seed_rows(n, k, seed)
    size = 2 * (n // (2 * k))
    assert size >= 2
    labels = np.concatenate([np.repeat(np.arange(k), size - 1), np.zeros(n - k * size, dtype=np.int64)])
    member = np.empty(n, np.int32)
    member[np.setdiff1d(np.arange(n), rows)] = rng.permutation(labels)
    member[rows] = np.arange(k)
    gap = 10.0 if d <= 16 else 100.0
    x = rng.uniform(1.0, 2.0, size=(n, d)).astype(F32)
    x[:, 0] = (gap * (member % 32) + rng.uniform(-0.1, 0.1, n)).astype(F32)
    x[:, 1] = (gap * (member // 32) + rng.uniform(-0.1, 0.1, n)).astype(F32)
    for c in range(k):
        idx = np.flatnonzero(member == c)
        for col, f in payload.items():
            x[idx, col] = f(len(idx), rng)
    return x, member


def test_kmeans_unclaimed_rows(amd, orc):
    """route: rows no centroid claims (a NaN row, an inf coordinate, a row at distance >= 2^32 from everything) in both update paths --
    kmeans_scatter_lds_kernel's `c < 0` (n = 5000) and the ballot of kmeans_update_kernel (n = 3000) -- and, through opq_train, in
    kmeans_residual_kernel, which reads them against centroid 0.  The rows are kept off the seed rows, so no centroid starts as one."""
    for n in (5000, 3000):
        rng = np.random.default_rng(n)
        k, d = 16, 12
        x, member = designed(rng, n, k, d, 1, {})
        bad = np.setdiff1d(np.arange(n), seed_rows(n, k, 1))[[0, 7, 100, n - 20]]
        x[bad[0]] = np.nan
        x[bad[1], 3] = np.inf
        x[bad[2], 0] += F32(1e6)
        x[bad[3], d - 1] = np.nan
        member[bad] = -1
        oc, oa, gc, ga = check_kmeans(amd, orc, x, k, 2, seeds=(1,))
        assert np.array_equal(oa, member)                   # (the oracle follows the design: the four rows get -1)
        oc, ob = orc.opq_train(x, 4, 2, 16, 2, 1)
        gc, gb = amd.opq_train(x, 4, 2, 16, 2, 1)
        assert np.array_equal(bits(gc), bits(oc)) and np.array_equal(bits(gb), bits(ob))


@pytest.mark.parametrize("k", [1, 3])
def test_kmeans_large_cluster(amd, orc, k):
    """route: the scatter update with m ~ 1e5 .. 3e5 members per cluster (n = 300 000, d = 2), where the 2 m 2^-53 factor of the proof's
    bound carries weight (and k = 1 puts every LDS atomic of a workgroup on one address); bit parity with the index-order sum"""
    rng = np.random.default_rng(k)
    n = 300_000
    blob = rng.choice(3, size=n, p=[0.6, 0.3, 0.1])
    x = (np.array([[5, 1], [-7, 3], [2, -9]], F32)[blob] + rng.normal(size=(n, 2))).astype(F32)
    check_kmeans(amd, orc, x, k, 2, device=(k == 3))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the proof of the scatter update (kmeans_finalize_kernel), forced both ways
# ---------------------------------------------------------------------------------------------------------------------
A_EVEN = F32(1.5)                           # even mantissa: the tie a + ulp / 2 rounds to a
A_ODD = np.nextafter(A_EVEN, F32(2))        # odd mantissa: the tie a + ulp / 2 rounds to a + ulp
TINY = F32(2.0 ** -120)


def _halves(lo, hi):
    def f(m, rng):
        return rng.permutation(np.array([lo] * (m // 2) + [hi] * (m - m // 2), F32))
    return f


def _cancel_odd_one_out(m, rng):
    """+v and -v in pairs, v in [1, 2), and one or two values left over"""
    v = rng.uniform(1.0, 2.0, (m - 1) // 2).astype(F32)
    return rng.permutation(np.concatenate([v, -v, rng.uniform(1.0, 2.0, m - 2 * len(v)).astype(F32)]))


def _cancel_over_tiny(m, rng):
    """+v and -v in pairs, v in [1, 2), among values near 2^-40: the mean is the tiny values' and every addition next to a v rounds,
    so the low bits of the double sum, and with them the float, depend on the order"""
    v = rng.uniform(1.0, 2.0, m // 3).astype(F32)
    return rng.permutation(np.concatenate([v, -v, (rng.uniform(1.0, 2.0, m - 2 * len(v)) * 2.0 ** -40).astype(F32)]))


def _const(value):
    def f(m, rng):
        return np.full(m, value, F32)
    return f


PAYLOADS = {
    "midpoint": (_halves(A_EVEN, np.nextafter(A_EVEN, F32(2))), _halves(A_ODD, np.nextafter(A_ODD, F32(2)))),
    "tiny": (_halves(TINY, -TINY), _halves(-TINY, TINY)),
    "cancel": (_cancel_odd_one_out, _cancel_over_tiny),
    "zeros": (_const(-0.0), _const(0.0)),
}


def check_designed(amd, orc, kind, n, k, d, device=False):
    """k-means of designed rows with the payload `kind` in the last two coordinates, niter = 1 (assign to the seeds, one update, assign):
    the oracle's assignment is the designed membership, the library equals the oracle, and the payload centroids of the clusters
    with an even count are the values derived in the tests' docstrings"""
    rng = np.random.default_rng(n + k + d + len(kind))
    cols = (d - 2, d - 1)
    x, member = designed(rng, n, k, d, 1, dict(zip(cols, PAYLOADS[kind])))
    oc, oa, gc, ga = check_kmeans(amd, orc, x, k, 1, seeds=(1,), device=device)
    assert np.array_equal(oa, member)
    even = np.bincount(member, minlength=k) % 2 == 0
    assert even[1:].all()
    pay = gc[even][:, cols]
    if kind == "midpoint":
        assert (pay[:, 0] == A_EVEN).all() and (pay[:, 1] == np.nextafter(A_ODD, F32(2))).all()
    if kind in ("tiny", "zeros"):
        assert (pay == 0).all()
        assert not np.signbit(pay).any(), np.argwhere(np.signbit(gc))[:10]
    if kind == "zeros":
        assert not np.signbit(gc[:, cols]).any()


@pytest.mark.parametrize("n,k", [(4096, 1), (4096, 4), (5120, 512)])
def test_scatter_proof_exact_midpoints(amd, orc, n, k):
    """route: kmeans_finalize_kernel must REJECT (lo != hi) and kmeans_update_flagged_kernel decide.  Each cluster holds a and
    nextafter(a, +inf) in equal numbers, shuffled: every partial sum is exact in double and the mean is exactly halfway between two
    floats, so float((S - E) / m) = a and float((S + E) / m) = a + ulp whatever E > 0 is, and index order (here: exact) rounds half to
    even.  Column d - 2 has a = 1.5 (even mantissa): the centroid is a.  Column d - 1 has a = nextafter(1.5) (odd): the centroid is
    a + ulp.  A finalize that accepted lo fails on the second, one that accepted hi fails on the first."""
    check_designed(amd, orc, "midpoint", n, k, 4, device=(k == 4))


@pytest.mark.parametrize("n,k", [(4096, 1), (4096, 4), (5120, 512)])
def test_scatter_proof_cancelling_tiny_values(amd, orc, n, k):
    """route: kmeans_finalize_kernel's comparison of lo and hi at a sum of exactly zero.  Each cluster holds +2^-120 and -2^-120 in
    equal numbers: every partial sum is an exact multiple of 2^-120 and the index-order sum ends as x + (-x) = +0.0, so the centroid is
    +0.0f.  The scattered S is 0 too, E = 2 m 2^-53 sum|x| > 0, and (S - E) / m, (S + E) / m lie far below the smallest float
    denormal: lo = -0.0f, hi = +0.0f.  They compare equal as floats but are not the same float: a finalize that stores lo leaves
    -0.0f (it did, before lo and hi were compared as bit patterns)."""
    check_designed(amd, orc, "tiny", n, k, 4)


@pytest.mark.parametrize("n,k", [(4096, 1), (4096, 4), (5120, 512)])
def test_scatter_proof_heavy_cancellation(amd, orc, n, k):
    """route: kmeans_finalize_kernel rejecting on the WIDTH of [S - E, S + E]: sum|x| ~ 1.5 m against a sum of ~1 (column d - 2: +-v
    and an odd one out) or of ~m 2^-40 (column d - 1: +-v among tiny values, where the double sum itself depends on the order of the
    additions), so kmeans_update_flagged_kernel has to walk the members in ascending row order.  Parity with the oracle is the only
    assertion."""
    check_designed(amd, orc, "cancel", n, k, 4)


@pytest.mark.parametrize("n,k", [(4096, 1), (4096, 4), (5120, 512)])
def test_scatter_proof_signed_zero_columns(amd, orc, n, k):
    """route: a coordinate that is -0.0 in every row, and one that is +0.0: sum|x| = 0, so kmeans_scatter_lds_kernel adds nothing and
    kmeans_finalize_kernel sees S = E = 0.  The index-order sum is 0.0 + (-0.0) + ... = +0.0: the centroid is +0.0f in both."""
    check_designed(amd, orc, "zeros", n, k, 4)


@pytest.mark.parametrize("n", [4096, 4097, 4607, 4608, 4609])
def test_flagged_walk_tail(amd, orc, n):
    """route: kmeans_update_flagged_kernel's walk of 8 x 64 assignments at a time and its n % 512 tail (0, 1, 511, 0, 1), with every
    centroid flagged by exact-midpoint payloads and members up to the last row"""
    check_designed(amd, orc, "midpoint", n, 4, 4)


@pytest.mark.parametrize("n,d", [(4097, 449), (4096, 512)])
def test_flagged_walk_wide_rows(amd, orc, n, d):
    """route: kmeans_update_flagged_kernel's last of KM_DPL = 8 slots per lane, with one lane in it (d = 449) and full (512): the
    exact-midpoint payloads sit in the last two coordinates"""
    check_designed(amd, orc, "midpoint", n, 4, d)


# ---------------------------------------------------------------------------------------------------------------------
# 4. training through the strided filter (ld = D, d = D / M)
# ---------------------------------------------------------------------------------------------------------------------
def flagging_rows(x, K, nan_row=True):
    """rows the filter cannot decide: seed row 1 = seed row 0 (two equal centroids from the start: every row near them ties), twenty
    duplicates of seed row 2, a NaN row"""
    n = x.shape[0]
    rows = seed_rows(n, K, 1)
    free = np.setdiff1d(np.arange(n), rows)
    x[rows[1]] = x[rows[0]]
    x[free[10:30]] = x[rows[2]]
    if nan_row:
        x[free[40]] = np.nan
    return x


@pytest.mark.parametrize("n,D,M,K,coarseK,device", [(4500, 128, 4, 64, 4, True), (4200, 96, 2, 80, 1, False),
                                                    (4100, 256, 2, 64, 3, False), (4100, 160, 2, 100, 2, False)])
def test_opq_train_strided_filter(amd, orc, n, D, M, K, coarseK, device):
    """route: the sub-space k-means of cvtmi_opq_train on the residual matrix in place (res + m * step, ld = D) with D / M = 32, 48, 128,
    80 >= 32, K >= 64, n >= 4096: assign_filter_kernel<2 / 3 / 8 / 5>, assign_gather_rows_kernel and the split / fold resolve all read
    rows at a stride (variant 0); variant 1 reads the same strided rows in kmeans_assign_reg_kernel.  D = 256, 160: the coarse k-means
    runs the generic kernel first."""
    rng = np.random.default_rng(n + D)
    x = flagging_rows(clustered(rng, n, D, 24), max(K, coarseK))
    oc, ob = orc.opq_train(x, coarseK, M, K, 2, 1)
    try:
        for variant in (0, 1):
            amd.set_tuning("assign_variant", variant)
            gc, gb = amd.opq_train(x, coarseK, M, K, 2, 1)
            assert np.array_equal(bits(gc), bits(oc)), variant
            assert np.array_equal(bits(gb), bits(ob)), (variant, np.argwhere(bits(gb) != bits(ob))[:10])
            if device:
                import torch
                tc, tb = amd.opq_train(torch.from_numpy(x).cuda(), coarseK, M, K, 2, 1)
                assert np.array_equal(bits(tc.cpu().numpy()), bits(oc)) and np.array_equal(bits(tb.cpu().numpy()), bits(ob)), variant
    finally:
        amd.set_tuning("assign_variant", 0)


def test_opq_learn_rotation_strided_filter(amd, orc):
    """route: the same strided sub-space k-means (D / M = 32, K = 64, n = 4200) behind the MFMA rotation of cvtmi_opq_learn_rotation,
    with rows that tie between equal centroids"""
    rng = np.random.default_rng(4200)
    n, D, M, K = 4200, 128, 4, 64
    A = rng.normal(size=(D, D))
    x = ((rng.normal(size=(n, D)) * np.exp(-np.arange(D) / (D / 5.0))) @ A.T).astype(F32)
    x = flagging_rows(x, K, nan_row=False)
    oR, ob = orc.opq_learn_rotation(x, M, K, 1, 2, 1)
    gR, gb = amd.opq_learn_rotation(x, M, K, 1, 2, 1)
    assert np.array_equal(bits(gR), bits(oR)) and np.array_equal(bits(gb), bits(ob))
