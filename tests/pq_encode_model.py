"""What test_gpu_pq_encode_routes.py rests on, none of it needing a GPU:

1. a host copy of the PQ-encode dispatch (cvt_amd/csrc/opq_encode.hip: encm_lds, encm_ok, pq_encode_fuses_lists, pq_encode_takes_perm,
   launch_pq_encode, launch_coarse_assign; cvt_amd/csrc/api_opq.hip: cvtmi_opq_encode_dev, cvtmi_opq_rotate_encode_dev): from the model's
   shape (D, M, K, coarseK), its rotation (none / "perm" / "R"), encode_variant, the 16-byte alignment of the rows, the row count and the
   CU count to the ordered list of launches (name, grid, block, dynamic LDS) that cvt_amd.launch_log() must show, and the error code
   of the call;
2. the models (coarse centroids, codebooks) and the hard rows every matrix-core shape is encoded with, and the rows of the other routes;
3. the rows aimed at the single-list chain of the permuted route, with fp32 sequential sums of both summation orders;
4. the list of cases.

Hard rows (hard_rows).  Everything is built as a residual r and stored as x = coarse[l] + r, l = row % coarseK.  The centroids are
N(0, 1) draws rounded to multiples of 2^-14, and so are the codewords 40 and 41 of every sub-quantiser (and 3 and 17 of the first), so
that for these the sum and the difference are exact and a row "on a codeword" has exactly that residual.  With coarseK == 3 the codebooks are N(0, 0.05^2): the
residuals stay far smaller than the distance between two centroids and a row's list is the l it was built on (the oracle decides anyway).
The special rows come first, so that the first 31 .. 257 rows of the table already hold them:
  non-finite     a +inf, a -inf and a NaN entry (in the first and the last sub-quantiser, and in dimension step - 1 of one: the second
                 lane half at step 16), an all-NaN row
  zero           x = coarse[l]: an all-zero residual
  norm           |x - coarse[0]|^2 = 2^32 f for f = 1 -+ 1e-3, 1 - 2e-7, 1 - 1e-7, 1 - 6e-8, 1 - 3e-8, 1, 1 + 1e-7 (around the start value of
                 the argmin) and 0.49, 0.5, 0.51 (around the kernel's norm2 * 1.01 < 2^31 gate), two directions each
  ladder         sub-space 0 holds mid(a, b) + t (a - b) for its codewords a = 3 = (4 sigma, .. 4 sigma) and b = 17 = a + (0.75, 0, .. 0): 0.75
                 apart, and every other codeword much farther from the midpoint than they; D_b - D_a =
                 2 t |a - b|^2, and t is chosen so that (D_b - D_a) / Q = 0, -+2^-24, -+2^-22 .. -+2^-10 with Q = |r|^2 + max |c|^2 of
                 that sub-quantiser: rungs below, at and above the kernel's bound 1.5 * 2^-14 Q
  big / tiny     N(0, 1) residuals x 3e4 (distances pass float(UINT_MAX): code 255) and x 1e-30
  q30            one sub-space holds a residual of length 2^15 sqrt(1 -+ 1e-3) (and -+ 3e-3): Q either side of 2^30
  on a codeword  residual = codeword 40 / 41 of every sub-quantiser (201 is 41 one ulp up; in the "dup" codebook 200 is a copy of 40)
  cover          8 rows around every codeword j = 0 .. 255 (codeword + 0.1 sigma noise): every code value occurs in every sub-quantiser
Codebook passes (books_for_pass): "plain"; "dup" (codeword 200 = codeword 40: the first must win, so 200 never occurs -- which is why the
duplicates have a pass of their own, apart from the one that must show every code value); "inf" (one infinite coordinate in codeword
99 of every sub-quantiser: max |c|^2 is infinite, every pair takes the exact chain); "tiny" (the plain codebook x 1e-20: max |c|^2 is a
denormal, so for the zero and the tiny residuals Q < 2^-60)."""
import math

import numpy as np

F32 = np.float32
KB = 256                        # kBlock
ENCM_THREADS = 512
ENC_V = 4
ENCM_LDS_LIMIT = 160 * 1024
ENCM_MIN_ROWS = 1
START = F32(4294967296.0)       # float(UINT_MAX)
OK, EINVAL, EUNSUPPORTED = 0, -1, -5

MFMA, VALU, GENERIC = "pq_encode_mfma_kernel", "pq_encode_kernel", "pq_encode_generic_kernel"
COARSE, ASSIGN_REG = "coarse_assign_kernel", "kmeans_assign_reg_kernel"
PERMUTE, PERMUTE_WIDE, ROTATE = "permute_kernel", "permute_wide_kernel", "rotate_gemm_kernel"


# ---- 1. the dispatch ----

def blocks_for(count, per):
    return -(-count // per)


def encm_lds(M, step):
    return (M * 256 * step + M * 256 + M) * 4


def encm_ok(D, M, K, ax):
    """ax: the rows, the codebooks and the centroids are all 16-byte aligned (the handle's own two always are)"""
    step = D // M
    return K == 256 and step in (8, 16) and M <= 16 and D == M * step and encm_lds(M, step) <= ENCM_LDS_LIMIT and ax


def chooses_mfma(variant, n):
    return variant == 2 or (variant == 0 and n >= ENCM_MIN_ROWS)


def pq_encode_fuses_lists(D, M, K, coarseK, ax, n, variant):
    return coarseK == 1 and encm_ok(D, M, K, ax) and chooses_mfma(variant, n)


def pq_encode_takes_perm(D, M, K, rot, ax, n, variant):
    return rot == "perm" and D // M == 8 and encm_ok(D, M, K, ax) and chooses_mfma(variant, n)


def launch_pq_encode(D, M, K, ax, n, variant, cus, single_list_out=False, perm=False, coarseK=1, rot=None):
    """-> (launches, rc)"""
    step = D // M
    if n <= 0:
        return [], OK
    if perm and not pq_encode_takes_perm(D, M, K, rot, ax, n, variant):
        return [], EINVAL
    if K > 256:
        return [], EUNSUPPORTED
    mfma_ok = encm_ok(D, M, K, ax)
    if variant == 2 and not mfma_ok:
        return [], EUNSUPPORTED
    if single_list_out and not pq_encode_fuses_lists(D, M, K, coarseK, ax, n, variant):
        return [], EINVAL
    if mfma_ok and chooses_mfma(variant, n):
        grid = min(cus, blocks_for(blocks_for(n, 32), ENCM_THREADS // 64))
        return [(MFMA, (grid, 1, 1), ENCM_THREADS, encm_lds(M, step))], OK
    if step in (2, 4, 8, 16, 32):
        return [(VALU, (blocks_for(n, KB * ENC_V), 1, 1), KB, 0)], OK
    return [(GENERIC, (blocks_for(n, KB), 1, 1), KB, 0)], OK


def coarse_assign_launches(D, coarseK, n):
    """launch_coarse_assign for the models of this file (fewer than 64 centroids: launch_kmeans_assign takes neither the matrix-core
    filter nor the split / fold path, whatever assign_variant says)"""
    assert coarseK < 64
    if n <= 0:
        return []
    return [(ASSIGN_REG if D <= 128 else COARSE, (blocks_for(n, KB), 1, 1), KB, 0)]


def encode_dev(D, M, K, coarseK, variant, ax, n, cus, lists=True):
    """cvtmi_opq_encode_dev -> (launches up to the failure, rc); lists: the caller passes a list_id array"""
    if n == 0:
        return [], OK
    want_lists = lists or coarseK > 1             # (coarseK > 1 without the caller's array: the handle's scratch)
    if want_lists and coarseK == 1 and pq_encode_fuses_lists(D, M, K, coarseK, ax, n, variant):
        return launch_pq_encode(D, M, K, ax, n, variant, cus, single_list_out=True, coarseK=coarseK)
    out = coarse_assign_launches(D, coarseK, n) if want_lists else []
    more, rc = launch_pq_encode(D, M, K, ax, n, variant, cus, coarseK=coarseK)
    return out + more, rc


def rotate_launches(D, rot, n):
    """opq_rotate_impl into the handle's (16-byte aligned) scratch"""
    if rot == "perm":
        narrow = (D % 4 == 0 and D // 4 <= KB) or D <= KB
        return [(PERMUTE if narrow else PERMUTE_WIDE, (256 * 8, 1, 1), KB, 0)], OK
    if D % 32 != 0 or D < 32 or D > 128:
        return [], EUNSUPPORTED
    lds = (D * (D + 1) + (512 // 64) * 2 * 32 * 33) * 4
    return [(ROTATE, (min(256, blocks_for(blocks_for(n, 32), 8)), 1, 1), 512, lds)], OK


def rotate_encode_dev(D, M, K, coarseK, rot, variant, ax, n, cus, lists=True):
    """cvtmi_opq_rotate_encode_dev -> (launches up to the failure, rc); rot: None, "perm" or "R" """
    if n == 0:
        return [], OK
    if rot is None:
        return encode_dev(D, M, K, coarseK, variant, ax, n, cus, lists)
    if rot == "perm" and coarseK == 1 and pq_encode_takes_perm(D, M, K, rot, ax, n, variant):
        return launch_pq_encode(D, M, K, ax, n, variant, cus, single_list_out=lists, perm=True, coarseK=coarseK, rot=rot)
    out, chunk = [], 131072
    for a in range(0, n, chunk):
        m = min(chunk, n - a)
        more, rc = rotate_launches(D, rot, m)
        out += more
        if rc != OK:
            return out, rc
        more, rc = encode_dev(D, M, K, coarseK, variant, True, m, cus, lists)
        out += more
        if rc != OK:
            return out, rc
    return out, OK


def instance(D, M, K, coarseK, rot, variant, ax, n, entry="encode"):
    """the template instance behind the pq_encode* record of a call that succeeds (the log holds the plain name only)"""
    step = D // M
    if entry == "rotate_encode" and rot is not None:
        if coarseK == 1 and pq_encode_takes_perm(D, M, K, rot, ax, n, variant):
            return "pq_encode_mfma_kernel<8, PERM>"
        ax = True                                          # the rotated rows lie in the handle's aligned scratch
    if encm_ok(D, M, K, ax) and chooses_mfma(variant, n):
        return "pq_encode_mfma_kernel<%d>" % step
    return "pq_encode_kernel<%d>" % step if step in (2, 4, 8, 16, 32) else GENERIC


# ---- 2. models and rows ----

GRID = 2.0 ** -14
NORM_F = [1 - 1e-3, 1 - 2e-7, 1 - 1e-7, 1 - 6e-8, 1 - 3e-8, 1.0, 1 + 1e-7, 1 + 1e-3, 0.49, 0.5, 0.51]
LADDER_V = [0.0] + [s * 2.0 ** -e for e in range(24, 8, -2) for s in (1, -1)]
Q30_F = [1 - 1e-3, 1 + 1e-3, 1 - 3e-3, 1 + 3e-3]
PASSES = ("plain", "dup", "inf", "tiny")
COVER = 8


def on_grid(a):
    return (np.round(np.asarray(a, np.float64) / GRID) * GRID).astype(F32)


def model(D, M, K, coarseK):
    """(coarse [coarseK][D], books [M][K][step]) of one shape; deterministic"""
    rng = np.random.default_rng(D * 10_007 + M * 101 + K + coarseK)
    step = D // M
    sigma = 0.05 if coarseK > 1 else 1.0
    coarse = on_grid(rng.standard_normal((coarseK, D)))
    books = (rng.standard_normal((M, K, step)) * sigma).astype(F32)
    if K == 256:
        for j in (40, 41):
            books[:, j] = on_grid(books[:, j])
        books[0, 3] = on_grid(np.full(step, 4 * sigma))       # the ladder's pair: clear of the cloud, so that nothing else is near its midpoint
        books[0, 17] = books[0, 3]
        books[0, 17, 0] += F32(0.75)
        books[:, 201] = np.nextafter(books[:, 41], F32(np.inf))
    return coarse, np.ascontiguousarray(books)


def books_for_pass(books, which):
    b = books.copy()
    M, K, step = b.shape
    if which == "dup":
        b[:, 200] = b[:, 40]
    elif which == "inf":
        for m in range(M):
            b[m, 99, m % step] = np.inf
    elif which == "tiny":
        b = (b * F32(1e-20)).astype(F32)
    else:
        assert which == "plain"
    return np.ascontiguousarray(b)


def flat(books, j):
    """codeword j of every sub-quantiser, as one row"""
    return books[:, j, :].reshape(-1)


def hard_table(D, M, coarseK):
    """the table of the module docstring for a K = 256 model -> (x [n][D] fp32 (n = 2162; 2158 with M = 1), {group: row indices})"""
    coarse, books = model(D, M, 256, coarseK)
    step = D // M
    sigma = 0.05 if coarseK > 1 else 1.0
    rng = np.random.default_rng(D * 977 + M * 13 + coarseK)
    res, groups, mark = [], {}, [0]

    def group(name):
        groups[name] = np.arange(mark[0], len(res))
        mark[0] = len(res)

    def ordinary():
        return (flat(books, int(rng.integers(0, 256))) + 0.3 * sigma * rng.standard_normal(D)).astype(F32)

    # non-finite
    for pos, v in ((min(5, D - 1), np.inf), (D - 3, -np.inf), (step - 1, np.nan), (D - 1, np.nan), (D - step, np.inf)):
        r = ordinary()
        r[pos] = v
        res.append(r)
    res.append(np.full(D, np.nan, F32))
    group("nonfinite")
    # zero residual
    res += [np.zeros(D, F32) for _ in range(6)]
    group("zero")
    # |x - coarse[0]|^2 = 2^32 f
    norm_rows = []
    for f in NORM_F:
        for _ in range(2):
            v = rng.standard_normal(D)
            norm_rows.append(len(res))
            res.append(v / np.linalg.norm(v) * math.sqrt(2.0 ** 32 * f))          # float64: rounded once, in x
    group("norm")
    # ladder across the decision bound, sub-space 0
    a, b = books[0, 3].astype(np.float64), books[0, 17].astype(np.float64)
    e = a - b
    mid = (a + b) / 2
    cmax = float(np.max(np.sum(books[0].astype(np.float64) ** 2, axis=1)))
    for v in LADDER_V:
        for _ in range(2):
            r = ordinary().astype(np.float64)
            t = v * (float(mid @ mid) + cmax) / (2 * float(e @ e))
            r[:step] = mid + t * e
            res.append(r)
    group("ladder")
    # big and tiny residuals
    res += [rng.standard_normal(D) * 3e4 for _ in range(12)]
    group("big")
    res += [rng.standard_normal(D) * 1e-30 for _ in range(6)]
    group("tiny")
    # Q either side of 2^30
    for f in Q30_F:
        for m in sorted({0, M - 1}):
            r = ordinary().astype(np.float64)
            u = rng.standard_normal(step)
            r[m * step:(m + 1) * step] = u / np.linalg.norm(u) * 2.0 ** 15 * math.sqrt(f)
            res.append(r)
    group("q30")
    # on a codeword
    res += [flat(books, 40) for _ in range(8)]
    group("on40")
    res += [flat(books, 41) for _ in range(8)] + [flat(books, 201) for _ in range(4)]
    group("on41")
    n_special = len(res)
    # around every codeword
    for j in range(256):
        for _ in range(COVER):
            res.append(flat(books, j) + 0.1 * sigma * rng.standard_normal(D))
    n = len(res)
    lists = np.arange(n) % coarseK
    lists[norm_rows] = 0
    with np.errstate(all="ignore"):
        x = (coarse[lists].astype(np.float64) + np.stack([np.asarray(r, np.float64) for r in res])).astype(F32)
    group("cover")
    assert n_special < 160
    return x, groups


def hard_rows(D, M, coarseK):
    return hard_table(D, M, coarseK)[0]


def plain_rows(D, M, K, coarseK, n):
    """rows for the VALU and generic routes (any K, any step): clustered residuals, and at the head a NaN row, an inf entry, a zero
    residual, a row on codeword 1 of every sub-quantiser, a residual x 3e4 and |x - coarse[0]|^2 = 2^32 (1 -+ 1e-3)"""
    coarse, books = model(D, M, K, coarseK)
    rng = np.random.default_rng(D * 31 + M * 7 + K + n)
    pick = rng.integers(0, K, size=(n, M))
    r = books[np.arange(M)[None, :], pick].reshape(n, D).astype(np.float64) + 0.3 * (0.05 if coarseK > 1 else 1.0) * rng.standard_normal((n, D))
    lists = np.arange(n) % coarseK
    head = [np.full(D, np.nan), None, np.zeros(D), flat(books, 1).astype(np.float64), rng.standard_normal(D) * 3e4]
    for f in (1 - 1e-3, 1 + 1e-3):
        v = rng.standard_normal(D)
        head.append(v / np.linalg.norm(v) * math.sqrt(2.0 ** 32 * f))
    for i, h in enumerate(head):
        if i < n:
            if h is None:
                r[i, D // 2] = np.inf
            else:
                r[i] = h
            if i >= 5:
                lists[i] = 0
    with np.errstate(all="ignore"):
        return (coarse[lists].astype(np.float64) + r).astype(F32)


def wrap_rows(hard, n):
    """n rows that walk the hard table over and over -> (x, the index of every row in the table)"""
    idx = (np.arange(n) + 3) % hard.shape[0]
    return np.ascontiguousarray(hard[idx]), idx


# ---- 3. the permuted route ----

def perms(D):
    """the three kinds of map cvtmi_opq_create accepts: a random permutation (with perm[D / 2] != D / 2: centroid_rows needs it), the
    identity, a map with repeated indices"""
    seed = D
    while True:
        p = np.random.default_rng(seed).permutation(D).astype(np.int32)
        if D == 1 or p[D // 2] != D // 2:
            break
        seed += 1000
    rep = np.random.default_rng(D + 7).integers(0, D, size=D).astype(np.int32)
    return {"random": p, "identity": np.arange(D, dtype=np.int32), "repeated": rep}


def unpermute(y, perm):
    """raw rows x with x[:, perm] as close to y as the map allows (equal for a permutation; columns the map never reads hold 0.25)
    -> (x, x[:, perm])"""
    x = np.full_like(y, F32(0.25))
    x[:, perm] = y
    return x, np.ascontiguousarray(x[:, perm])


def seq_sum_sq(d):
    """fp32 sum of d^2 over the columns in index order: one rounded product and one rounded addition per column"""
    with np.errstate(all="ignore"):
        sq = d * d
        assert sq.dtype == F32
        return np.add.accumulate(sq, axis=1, dtype=F32)[:, -1]


def chain_lists(x, coarse0):
    """the single-list decision of the reference on rows x (IVFOPQ.cpp:110-129 with one centroid), by fp32 sequential sums"""
    with np.errstate(all="ignore"):
        return np.where(seq_sum_sq(x - coarse0[None, :]) < START, 0, -1).astype(np.int32)


ORDER_SEED = 1


def order_rows(D, n=64):
    """raw rows with |x|^2 = 2^32 (1 - 3e-8 .. 1 - 2e-7), for a model with a zero centroid: the sum is within a few ulps (256) of the start
    value, so the order of the additions decides"""
    rng = np.random.default_rng(ORDER_SEED + D)
    v = rng.standard_normal((n, D))
    f = 1 - np.linspace(3e-8, 2e-7, n)
    return (v / np.linalg.norm(v, axis=1)[:, None] * np.sqrt(2.0 ** 32 * f)[:, None]).astype(F32)


def centroid_rows(D, perm):
    """(coarse0, raw rows [2][D]) for a permutation without fixed points: coarse0[j0] = 1e4 (the rest N(0, 1) on the grid).
    Row 0: x[perm[j0]] = 7e4, else x[:, perm] = coarse0 -- the reference sums (7e4 - 1e4)^2 = 3.6e9 < 2^32: list 0; in natural order the
    same value meets an ordinary centroid entry, (7e4 - c)^2 = 4.9e9: -1.
    Row 1: x[perm[j0]] = -6e4 and x[j0] = 1e4 -- the reference sums (-6e4 - 1e4)^2 = 4.9e9: -1; natural order 3.6e9 + (1e4 - 1e4)^2: list 0."""
    rng = np.random.default_rng(D + 99)
    j0 = D // 2
    inv = np.argsort(perm)
    assert perm[j0] != j0 and perm[inv[j0]] == j0
    coarse0 = on_grid(rng.standard_normal(D))
    coarse0[j0] = F32(1e4)
    y = np.stack([coarse0, coarse0]).astype(F32)
    y[0, j0] = F32(7e4)
    y[1, j0] = F32(-6e4)
    y[1, inv[j0]] = F32(1e4)                                  # x[j0] = y[inv[j0]]
    x, back = unpermute(y, perm)
    assert np.array_equal(back, y)
    return coarse0, x


# ---- 4. the cases: (D, M, K, coarseK) ----

MFMA8 = [(8, 1, 256, 1), (24, 3, 256, 1), (32, 4, 256, 3), (96, 12, 256, 1), (128, 16, 256, 1)]
MFMA16 = [(32, 2, 256, 1), (64, 4, 256, 3), (128, 8, 256, 1), (144, 9, 256, 1), (144, 9, 256, 3)]
MFMA_ROWS = [1, 31, 32, 33, 255, 256, 257]
WRAP = [(24, 3, 256, 1), (128, 16, 256, 1)]                 # n = 256 CUs + 257
REFUSED = [(160, 10, 256, 1), (256, 16, 256, 1)]
VALU_CASES = [(32, 16, 256, 1), (64, 16, 256, 2), (32, 4, 200, 1), (128, 4, 256, 1)]     # steps 2, 4, 8 (K = 200), 32
GENERIC_CASES = [(96, 2, 17, 3), (15, 3, 256, 1)]
MISALIGNED = [(128, 16, 256, 1), (128, 8, 256, 1), (64, 4, 256, 3)]
MISALIGNED_PERM = [(24, 3, 256, 1), (128, 16, 256, 1)]
PERM_CASES = [s for s in MFMA8 if s[3] == 1]
ORDER_D = [(96, 12), (128, 16)]
PLAIN_N = 1300                                             # two workgroups of the VALU kernel, the second ragged


def wrap_n(cus):
    return 256 * cus + 257
