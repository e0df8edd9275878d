"""The four small dense kernels every row and every query passes first, at their slab, tail and width edges, against the oracle:
the permutation gather (csrc/rotate.hip, launch_permute: permute_kernel<4>, permute_kernel<1>, permute_wide_kernel) == orc.reorder,
the dense rotation (rotate_gemm_kernel<NT>) == orc.rotate_fma, the distance tables (csrc/opq_encode.hip, lut_kernel and
lut8_kernel<4, 8 | 16 | 32>) == orc.lut, and the PCA projection (csrc/pca.hip) == orc.pca_project(..., flavour=1).

One comparison rule (first_mismatch): where the reference is not NaN the kernel's value has the same bits (signed zeros, infinities
and subnormals included); where it is NaN the kernel's is a NaN of any sign and payload.  The gather does no arithmetic and is held
bit for bit throughout, payloads included.  tests/test_dense_prologue_compare.py runs the rule on numpy arrays alone."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

F32 = np.float32
FLT_MAX = np.finfo(F32).max


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()  # raises if the HIP library is missing: there is no fallback
    return cvt_amd


# ---------------------------------------------------------------------------------------------------------------------
# the comparison rule
# ---------------------------------------------------------------------------------------------------------------------
def _rows(a):
    a = np.ascontiguousarray(a, dtype=F32)
    return a.reshape(a.shape[0], int(np.prod(a.shape[1:], dtype=np.int64)))


def first_mismatch(got, ref, nan_payload=False):
    """None, or (row, slab = row // 32, column) of the first element of `got` that breaks the rule against `ref`: equal bits where
    ref is not NaN, any NaN where ref is NaN (nan_payload=True: equal bits everywhere -- the gather).  Arrays of more than two
    dimensions are taken as rows of their first one (column = flat index inside the row)."""
    assert np.shape(got) == np.shape(ref), "shape %r != %r" % (np.shape(got), np.shape(ref))
    g, r = _rows(got), _rows(ref)
    bad = bits(g) != bits(r)
    if not nan_payload:
        bad &= ~(np.isnan(g) & np.isnan(r))
    rows = np.flatnonzero(bad.any(axis=1))
    if rows.size == 0:
        return None
    row = int(rows[0])
    return row, row // 32, int(np.flatnonzero(bad[row])[0])


def assert_same(got, ref, what, nan_payload=False):
    m = first_mismatch(got, ref, nan_payload)
    if m is not None:
        row, slab, col = m
        g, r = _rows(got)[row, col], _rows(ref)[row, col]
        raise AssertionError("%s: row %d (slab %d) column %d is %r (0x%08x), the reference has %r (0x%08x)"
                             % (what, row, slab, col, g, int(bits(g).ravel()[0]), r, int(bits(r).ravel()[0])))


def assert_within_1ulp(got, ref, what):
    """the normalised projection: NaN where the reference is NaN, elsewhere at most one ulp from it (what test_gpu_pca.py allows:
    the kernel adds the squares of a row as a tree, the reference in column order)"""
    g, r = _rows(got), _rows(ref)
    assert g.shape == r.shape
    gn, rn = np.isnan(g), np.isnan(r)
    ig = g.view(np.int32).astype(np.int64); ir = r.view(np.int32).astype(np.int64)
    ig = np.where(ig < 0, -(ig & 0x7FFFFFFF), ig); ir = np.where(ir < 0, -(ir & 0x7FFFFFFF), ir)
    bad = (gn != rn) | (~rn & (np.abs(ig - ir) > 1))
    rows = np.flatnonzero(bad.any(axis=1))
    if rows.size:
        row = int(rows[0]); col = int(np.flatnonzero(bad[row])[0])
        raise AssertionError("%s: row %d (slab %d) column %d is %r, the reference has %r" % (what, row, row // 32, col, g[row, col], r[row, col]))


# ---------------------------------------------------------------------------------------------------------------------
# 1. dense rotation: OpqIndex(..., R=R).rotate on device tensors == orc.rotate_fma
# ---------------------------------------------------------------------------------------------------------------------
def slab_plan(n):
    """launch_rotate_gemm: a wave owns 32-row slabs, blocks = min(256, ceil(slabs / 8)) workgroups of 8 waves, wave w walks slabs
    w, w + waves, w + 2 waves, ...  -> (slabs, waves, slabs walked by each wave, live rows of the last slab)"""
    slabs = (n + 31) // 32
    blocks = min(256, (slabs + 7) // 8)
    waves = 8 * blocks
    return slabs, waves, [len(range(w, slabs, waves)) for w in range(waves)], n - 32 * (slabs - 1)


_sift = {}


def sift_rows(D, n):
    """SIFT-like rows (finite, >= +0), generated once per width on the device: (device tensor, numpy copy) of the first n"""
    import torch
    from cvt_amd import synth
    if D not in _sift:
        x = synth.sift_like(131249, D, device="cuda")
        torch.cuda.synchronize()
        _sift[D] = (x, x.cpu().numpy())
    x, xh = _sift[D]
    return x[:n].contiguous(), xh[:n]


def dense_model(amd, D, R):
    return amd.OpqIndex(np.zeros((1, D), F32), np.zeros((1, 1, D), F32), R=R)


def check_rotation(amd, orc, D, n, seed):
    from cvt_amd import synth
    x, xh = sift_rows(D, n)
    R = synth.random_rotation(D, seed)
    y = dense_model(amd, D, R).rotate(x).cpu().numpy()
    assert_same(y, orc.rotate_fma(R, xh), "dense rotation D=%d n=%d" % (D, n))
    # a 0/1 permutation matrix: on finite rows the fmaf chain is the gather itself (every row, no oracle time)
    p = synth.random_permutation(D, seed + 1)
    P = np.zeros((D, D), F32)
    P[np.arange(D), p] = 1
    yp = dense_model(amd, D, P).rotate(x).cpu().numpy()
    assert_same(yp, xh[:, p], "0/1 rotation D=%d n=%d" % (D, n), nan_payload=True)


@pytest.mark.parametrize("D,n", [(128, 131249), (32, 131249), (64, 65649), (96, 65649)])
def test_rotation_several_slabs_per_wave(amd, orc, D, n):
    """The launcher caps the grid at 256 workgroups of 8 waves (slab_plan), so a wave walks a second slab only past 65 536 rows and a
    third past 131 072: the double-buffered accumulators, the stores issued between the next slab's matrix instructions and both
    epilogues.  n = 131 249: 4102 slabs, waves 0..5 walk three (A, B, A: the pending-A epilogue), the rest two (pending-B), the last
    slab is a third slab of 17 live rows.  n = 65 649: 2052 slabs, waves 0..3 walk two, the last slab has 17 live rows."""
    slabs, waves, per_wave, live = slab_plan(n)
    assert waves == 2048 and live == 17
    if n == 131249:
        assert slabs == 4102 and per_wave[:6] == [3] * 6 and set(per_wave[6:]) == {2} and (slabs - 1) % waves == 5
    else:
        assert slabs == 2052 and per_wave[:4] == [2] * 4 and set(per_wave[4:]) == {1} and (slabs - 1) % waves == 3
    check_rotation(amd, orc, D, n, seed=D + 1)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 255, 257])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_rotation_small_grids(amd, orc, D, n):
    """one partial or full slab, a grid of fewer slabs than one workgroup's eight waves (n <= 255) or one slab into a second
    workgroup (n = 257), tail rows clamped to n - 1; every width = every NT instantiation"""
    slabs, waves, per_wave, live = slab_plan(n)
    assert max(per_wave) == 1 and live == (n - 1) % 32 + 1
    assert (slabs <= 8 and waves == 8) if n <= 255 else (slabs == 9 and waves == 16)
    check_rotation(amd, orc, D, n, seed=100 * D + n)


def test_rotation_hard_values(amd, orc):
    """D = 128, n = 65 649 (waves 0..3 walk two slabs): NaN, +inf, -inf, both, subnormals, entries near FLT_MAX / D, zeros and -0.0
    rows in the first slab, in a second-generation slab (2049) and in the partial last one (2051, the last row among them: the row the
    clamped tail loads read).  The hard rows follow the rule against orc.rotate_fma; every other row is bit-exact -- a row's
    non-finite value does not reach its slab neighbours."""
    import torch
    from cvt_amd import synth
    D, n = 128, 65649
    slabs, waves, per_wave, live = slab_plan(n)
    assert slabs == 2052 and waves == 2048 and per_wave[:4] == [2] * 4 and live == 17
    x, xh = sift_rows(D, n)
    xh = xh.copy()
    rng = np.random.default_rng(0xD15E)
    base = xh[1000:1008].copy()
    hard = {
        "nan": np.full(D, np.nan, F32),
        "pinf": base[0], "ninf": base[1], "both": base[2],
        "subnormal": (rng.integers(1, 1 << 21, D, dtype=np.uint32) | (rng.integers(0, 2, D, dtype=np.uint32) << 31)).view(F32),
        "big": (rng.uniform(0.5, 1.0, D) * rng.choice([-1.0, 1.0], D) * (float(FLT_MAX) / D)).astype(F32),
        "zero": np.zeros(D, F32),
        "negzero": np.full(D, -0.0, F32),
    }
    hard["pinf"][17] = np.inf
    hard["ninf"][90] = -np.inf
    hard["both"][3] = np.inf; hard["both"][100] = -np.inf
    starts = [3, 2049 * 32 + 5, n - len(hard)]
    assert starts[2] >= 2051 * 32
    where = {}
    for s in starts:
        for i, (name, row) in enumerate(hard.items()):
            xh[s + i] = row
            where.setdefault(name, []).append(s + i)
    hard_rows = np.array(sorted(r for rows in where.values() for r in rows))
    R = synth.random_rotation(D, 77)
    ref = orc.rotate_fma(R, xh)
    # what the reference holds on these rows (so the rule below is applied to what the docstring says)
    plain = np.ones(n, bool); plain[hard_rows] = False
    assert np.isfinite(ref[plain]).all()
    assert np.isnan(ref[where["nan"]]).all() and np.isnan(ref[where["both"]]).any()
    assert np.isinf(ref[where["pinf"]]).all() and np.isinf(ref[where["ninf"]]).all()
    assert (bits(ref[where["zero"]]) == 0).all() and (bits(ref[where["negzero"]]) == 0).all()
    sub = ref[where["subnormal"]]
    assert (np.abs(sub) < np.finfo(F32).tiny).all() and (sub != 0).any()
    assert np.isfinite(ref[where["big"]]).all() and np.abs(ref[where["big"]]).max() > float(FLT_MAX) / D
    y = dense_model(amd, D, R).rotate(torch.from_numpy(xh).cuda()).cpu().numpy()
    assert_same(y[hard_rows], ref[hard_rows], "hard rows %s" % hard_rows.tolist())
    assert_same(y, ref, "rows around the hard ones")


# ---------------------------------------------------------------------------------------------------------------------
# 2. permutation: OpqIndex(..., perm=p).rotate == orc.reorder, bit for bit on random 32-bit patterns
# ---------------------------------------------------------------------------------------------------------------------
K_BLOCK = 256        # csrc/common.h kBlock
PERMUTE_GRID = 2048  # launch_permute: 256 * 8 workgroups


def permute_kernel_of(D, y_addr=0):
    """the three conditions of launch_permute, as written there"""
    if (D & 3) == 0 and D // 4 <= K_BLOCK and (y_addr & 15) == 0:
        return "permute_kernel<4>"
    elif D <= K_BLOCK:
        return "permute_kernel<1>"
    else:
        return "permute_wide_kernel"


def _sweep(D, vec):
    """rows one sweep of the whole grid covers: TY = kBlock / (D / VEC) rows per workgroup (one for the wide kernel)"""
    return PERMUTE_GRID * (K_BLOCK // (D // vec) if vec else 1)


def _shape(kernel, D, n, y_off=0):
    assert permute_kernel_of(D, y_off) == kernel, "D=%d y_off=%d no longer reaches %s" % (D, y_off, kernel)
    short = {"permute_kernel<4>": "vec4", "permute_kernel<1>": "scalar", "permute_wide_kernel": "wide"}[kernel]
    return pytest.param(D, n, y_off, id="%s-D%d-n%d%s" % (short, D, n, "-misaligned" if y_off else ""))


PERMUTE_SHAPES = [
    _shape("permute_kernel<4>", 128, 32773),      # CG = 32, TY = 8: two full sweeps of 2048 * 8 rows plus 5
    _shape("permute_kernel<4>", 100, 20483),      # CG = 25, TY = 10, threads 250..255 idle; a second sweep plus 3
    _shape("permute_kernel<4>", 4, 524291),       # CG = 1, TY = 256: a second sweep plus 3
    _shape("permute_kernel<4>", 1024, 2051),      # CG = 256, TY = 1
    _shape("permute_kernel<1>", 30, 16389),       # CG = 30, TY = 8, threads 240..255 idle
    _shape("permute_kernel<1>", 7, 73731),        # TY = 36
    _shape("permute_kernel<1>", 1, 524291),       # TY = 256
    _shape("permute_kernel<1>", 255, 2051),       # TY = 1, thread 255 idle
    _shape("permute_kernel<1>", 128, 4101, 4),    # the output 4 bytes past a 16-byte boundary: the scalar kernel, TY = 2
    _shape("permute_wide_kernel", 258, 4097),     # D > 256, D % 4 != 0: a second sweep of the 2048 workgroups plus one row
    _shape("permute_wide_kernel", 1028, 4097),    # D > 1024
    _shape("permute_kernel<4>", 128, 0), _shape("permute_kernel<4>", 128, 1),
    _shape("permute_kernel<1>", 30, 0), _shape("permute_kernel<1>", 30, 1),
    _shape("permute_wide_kernel", 258, 0), _shape("permute_wide_kernel", 258, 1),
]
assert _sweep(128, 4) * 2 + 5 == 32773 and _sweep(100, 4) + 3 == 20483 and _sweep(4, 4) + 3 == 524291 and _sweep(1024, 4) + 3 == 2051
assert _sweep(30, 1) + 5 == 16389 and _sweep(7, 1) + 3 == 73731 and _sweep(1, 1) + 3 == 524291 and _sweep(255, 1) + 3 == 2051
assert _sweep(128, 1) + 5 == 4101 and _sweep(258, 0) * 2 + 1 == 4097


@pytest.mark.parametrize("D,n,y_off", PERMUTE_SHAPES)
def test_permutation(amd, orc, D, n, y_off):
    """a random bijection, the identity, the reversal and a map with repeated indices (cvtmi_opq_create checks the range only; the
    gather is defined for repeats) over rows of random 32-bit patterns: every NaN payload, infinity and subnormal moves unchanged"""
    import torch
    rng = np.random.default_rng(D * 1000003 + n)
    xh = rng.integers(0, 1 << 32, size=(n, D), dtype=np.uint32).view(F32)
    x = torch.from_numpy(xh).cuda()
    SENT = 0x5EA7BEEF   # the words in front of and behind the output
    perms = {"bijection": rng.permutation(D), "identity": np.arange(D), "reversal": np.arange(D)[::-1], "repeats": rng.integers(0, D, D)}
    for name, p in perms.items():
        p = np.ascontiguousarray(p, dtype=np.int32)
        idx = amd.OpqIndex(np.zeros((1, D), F32), np.zeros((1, 1, D), F32), perm=p)
        buf = torch.full((n * D + 8,), SENT, dtype=torch.int32, device="cuda")
        assert buf.data_ptr() % 16 == 0 and y_off in (0, 4)
        lead = 4 + y_off // 4                          # the output starts 16 (+ 4) bytes into the buffer
        y_addr = buf.data_ptr() + 4 * lead
        assert permute_kernel_of(D, y_addr) == permute_kernel_of(D, y_off)
        rc = amd.lib().cvtmi_opq_rotate_dev(idx.h, C.c_void_p(x.data_ptr()), C.c_int64(n), C.c_void_p(y_addr),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, amd.lib().cvtmi_last_error()
        out = buf.cpu().numpy()
        y = out[lead:lead + n * D].view(F32).reshape(n, D)
        what = "%s D=%d n=%d" % (name, D, n)
        assert_same(y, orc.reorder(p, xh), what, nan_payload=True)
        assert np.array_equal(bits(y), bits(xh[:, p])), what
        assert (out[:lead] == SENT).all() and (out[lead + n * D:] == SENT).all(), what + ": a word outside the output was written"


# ---------------------------------------------------------------------------------------------------------------------
# 3. distance tables: idx.lut (host and device pointers) == orc.lut per query
# ---------------------------------------------------------------------------------------------------------------------
LUT_MODELS = [(128, 16, 256), (128, 8, 256), (128, 4, 200), (64, 16, 256), (36, 12, 100)]   # steps 8, 16, 32 (lut8_kernel) and 4, 3
LUT_NQ = [1, 63, 64, 65, 67, 130]
LUT_MINUS_ONE = [0, 5, 62, 63, 64, 66, 129]    # list_id == -1 (clamped to list 0): the last query of every nq among them
COARSE_K = 5


def lut_kernel_of(D, M, nq):
    """launch_lut: the batched kernel takes steps 8, 16 and 32 from 64 queries on"""
    return "lut8_kernel" if D // M in (8, 16, 32) and nq >= 64 else "lut_kernel"


for _D, _M, _K in LUT_MODELS:
    assert [lut_kernel_of(_D, _M, nq) for nq in LUT_NQ] == ["lut_kernel"] * 2 + ["lut8_kernel" if _D == 128 else "lut_kernel"] * 4
assert all(nq - 1 in LUT_MINUS_ONE for nq in LUT_NQ) and [nq % 4 for nq in LUT_NQ[2:]] == [0, 1, 3, 2]

_lut_cases = {}


def oracle_tables(orc, q, coarse, books, lists):
    return np.stack([orc.lut(q[f], coarse[max(int(lists[f]), 0)], books) for f in range(len(q))])


def lut_case(amd, orc, model):
    """model, 130 queries, their lists and both reference tables: made once per model and left unchanged"""
    if model not in _lut_cases:
        D, M, K = model
        rng = np.random.default_rng(D * 10000 + M * 1000 + K)
        coarse = rng.normal(size=(COARSE_K, D)).astype(F32)
        books = (rng.normal(size=(M, K, D // M)) * 0.5).astype(F32)
        lists = (np.arange(130) % COARSE_K).astype(np.int32)
        lists[LUT_MINUS_ONE] = -1
        q = (coarse[np.maximum(lists, 0)] + rng.normal(size=(130, D)) * 0.7).astype(F32)
        idx = amd.OpqIndex(coarse, books)
        _lut_cases[model] = (idx, coarse, books, q, lists, oracle_tables(orc, q, coarse, books, lists),
                             oracle_tables(orc, q, coarse, books, np.zeros(130, np.int32)))
    return _lut_cases[model]


def both_entries(idx, q, lists):
    """idx.lut through the host-pointer and the device-pointer entry"""
    import torch
    yield "host", idx.lut(q, lists)
    dl = None if lists is None else torch.from_numpy(np.ascontiguousarray(lists)).cuda()
    yield "device", idx.lut(torch.from_numpy(np.ascontiguousarray(q)).cuda(), dl).cpu().numpy()


@pytest.mark.parametrize("nq", LUT_NQ)
@pytest.mark.parametrize("model", LUT_MODELS, ids=lambda m: "D%d-M%d-K%d" % m)
def test_lut(amd, orc, model, nq):
    """below and above the switch at 64 queries, a last group of 1, 3 and 2 live queries, coarseK = 5 with list_id cycling through
    the lists and -1 at some queries (the last one always), list_id = None, K < 256"""
    idx, coarse, books, q, lists, ref, ref0 = lut_case(amd, orc, model)
    for entry, got in both_entries(idx, q[:nq], lists[:nq]):
        assert_same(got, ref[:nq], "%s entry, %s, nq=%d" % (entry, lut_kernel_of(model[0], model[1], nq), nq))
    for entry, got in both_entries(idx, q[:nq], None):
        assert_same(got, ref0[:nq], "%s entry, list_id=None, nq=%d" % (entry, nq))


@pytest.mark.parametrize("model", LUT_MODELS, ids=lambda m: "D%d-M%d-K%d" % m)
def test_lut_kernels_agree(amd, orc, model):
    """the first 63 queries answered alone (lut_kernel) and as part of 64 (lut8_kernel at steps 8, 16, 32): equal bits"""
    idx, coarse, books, q, lists, ref, ref0 = lut_case(amd, orc, model)
    a = idx.lut(q[:63], lists[:63])
    b = idx.lut(q[:64], lists[:64])
    assert_same(b[:63], a, "63 of 64 against 63", nan_payload=True)


@pytest.mark.parametrize("nq", [7, 67])
@pytest.mark.parametrize("model", LUT_MODELS, ids=lambda m: "D%d-M%d-K%d" % m)
def test_lut_hard_queries(amd, orc, model, nq):
    """a NaN in one sub-vector (only that m of that query is NaN; the other queries of its group of four are untouched), +inf,
    subnormal residuals (a query equal to an all-zero centroid plus 1e-41, against codewords near 1e-20 whose squared differences
    are subnormal, and against an all-zero codeword), differences whose squares overflow to +inf"""
    D, M, K = model
    step = D // M
    rng = np.random.default_rng(D + M + K + nq)
    coarse = rng.normal(size=(COARSE_K, D)).astype(F32)
    coarse[4] = 0
    books = (rng.normal(size=(M, K, step)) * 0.5).astype(F32)
    books[:, 2] = (rng.uniform(0.5, 1.0, size=(M, step)) * 1e-20 * rng.choice([-1.0, 1.0], size=(M, step))).astype(F32)
    books[:, 3] = 0
    lists = (np.arange(nq) % COARSE_K).astype(np.int32)
    lists[nq - 1] = -1
    q = (coarse[np.maximum(lists, 0)] + rng.normal(size=(nq, D)) * 0.7).astype(F32)
    i_nan, i_inf, i_sub, i_ovf2, i_ovf = 1, 2, 4, 5, nq - 1     # (nq = 67: the last query is the third of a group with three live ones)
    assert len({i_nan, i_inf, i_sub, i_ovf, i_ovf2}) == 5 and lists[i_sub] == 4 and lists[i_ovf] == -1
    q[i_nan, 1 * step + step - 1] = np.nan
    q[i_inf, (M - 1) * step] = np.inf
    q[i_sub] = coarse[4] + F32(1e-41)
    q[i_ovf] = F32(2e19)
    q[i_ovf2] = F32(1.5e19)                        # one square is finite, two overflow
    ref = oracle_tables(orc, q, coarse, books, lists)
    nan_at = np.zeros((nq, M), bool); nan_at[i_nan, 1] = True
    assert np.array_equal(np.isnan(ref).any(axis=2), nan_at) and np.isnan(ref[i_nan, 1]).all()
    assert (ref[i_inf, M - 1] == np.inf).all() and np.isfinite(ref[i_inf, :M - 1]).all()
    tiny = float(np.finfo(F32).tiny)
    assert ((ref[i_sub, :, 2] > 0) & (ref[i_sub, :, 2] < tiny)).all() and (bits(ref[i_sub, :, 3]) == 0).all()
    assert (ref[i_ovf] == np.inf).all() and (ref[i_ovf2] == np.inf).all()
    untouched = oracle_tables(orc, q[[0, 3]], coarse, books, lists[[0, 3]])   # the NaN query's group mates, computed alone
    assert np.array_equal(bits(ref[[0, 3]]), bits(untouched))
    idx = amd.OpqIndex(coarse, books)
    for entry, got in both_entries(idx, q, lists):
        assert_same(got, ref, "%s entry, %s, nq=%d" % (entry, lut_kernel_of(D, M, nq), nq))
    idx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. PCA projection: amd.pca_project == orc.pca_project(..., flavour=1)
# ---------------------------------------------------------------------------------------------------------------------
def cnn_like(rng, n, d):
    x = np.maximum(rng.normal(size=(n, d)), 0).astype(F32) * rng.gamma(2.0, 1.0, size=(1, d)).astype(F32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)


def pca_model(rng, din, dout):
    e = (rng.normal(size=(dout, din)) / np.sqrt(din)).astype(F32)
    mean = rng.normal(0.02, 0.01, size=din).astype(F32)
    return mean, e


def check_projection(amd, orc, mean, e, x, what, modes=(False, True), ref=None):
    """both epilogues against the specification: bit for bit under the rule without the normalisation, NaN for NaN and 1 ulp with it"""
    out = {}
    for l2 in modes:
        y = amd.pca_project(mean, e, x, l2norm=l2)
        spec = orc.pca_project(mean, e, x, l2, flavour=1) if ref is None else ref[l2][:len(x)]
        if l2:
            assert_within_1ulp(y, spec, what + ", normalised")
        else:
            assert_same(y, spec, what + ", raw")
        out[l2] = y
    return out


_pca_tails = {}


@pytest.mark.parametrize("n", [1, 127, 128, 129, 385])
@pytest.mark.parametrize("din,dout", [(64, 32), (100, 33), (1024, 128)])
def test_pca_row_tails(amd, orc, din, dout, n):
    """rows per workgroup = 128: one row, one short of a workgroup, a full one, one row into a second, one row into a fourth"""
    if (din, dout) not in _pca_tails:
        rng = np.random.default_rng(din * 1000 + dout)
        mean, e = pca_model(rng, din, dout)
        x = cnn_like(rng, 385, din)
        _pca_tails[(din, dout)] = (mean, e, x, {l2: orc.pca_project(mean, e, x, l2, flavour=1) for l2 in (False, True)})
    mean, e, x, ref = _pca_tails[(din, dout)]
    check_projection(amd, orc, mean, e, x[:n], "%d -> %d, n=%d" % (din, dout, n), ref=ref)


@pytest.mark.parametrize("dout", [1, 32, 33, 64, 65, 96, 128, 160, 192, 224, 225, 256])
def test_pca_every_tile_count(amd, orc, dout):
    """NT = 1..8 accumulator tiles, each at a full and a one-past width, din = 36: one full and one padded K chunk, n = 129"""
    assert (dout + 31) // 32 in range(1, 9) and 36 % 32 != 0
    rng = np.random.default_rng(dout)
    mean, e = pca_model(rng, 36, dout)
    check_projection(amd, orc, mean, e, cnn_like(rng, 129, 36), "36 -> %d" % dout)


@pytest.mark.parametrize("din,dout", [(1024, 128), (100, 33)])
def test_pca_non_finite_rows_stay_confined(amd, orc, din, dout):
    """a NaN row, a row with +inf in column 50 and a row with +inf and -inf, each in turn at rows 0, 127, 128 and the last of 300:
    those rows follow the specification, every other row keeps the bits of a run without them"""
    n = 300
    rng = np.random.default_rng(din + dout)
    mean, e = pca_model(rng, din, dout)
    clean = cnn_like(rng, n, din)
    base = {l2: amd.pca_project(mean, e, clean, l2norm=l2) for l2 in (False, True)}
    at = [0, 127, 128, n - 1]
    other = np.ones(n, bool); other[at] = False

    def spoil(row, kind):
        if kind == 0:
            row[:] = np.nan
        elif kind == 1:
            row[50] = np.inf
        else:
            row[50] = np.inf; row[din - 7] = -np.inf

    for shift in range(3):
        x = clean.copy()
        for i, r in enumerate(at):
            spoil(x[r], (i + shift) % 3)
        got = check_projection(amd, orc, mean, e, x, "%d -> %d, non-finite rows (shift %d)" % (din, dout, shift))
        spec = orc.pca_project(mean, e, x, False, flavour=1)
        assert not np.isfinite(spec[at]).any() and np.isfinite(spec[other]).all()
        for l2 in (False, True):
            assert_same(got[l2][other], base[l2][other], "rows beside the non-finite ones (normalise=%s)" % l2, nan_payload=True)


@pytest.mark.parametrize("din", [20, 100, 64])
def test_pca_pad_columns(amd, orc, din):
    """din % 32 != 0 (20, 100; 64 is the control): the columns past din are loaded from a clamped address -- columns 0..3 of the same
    row -- and must enter the products as exact zeros on BOTH operands.  +inf in x[r][0], -inf in x[r][3] and +inf in E[2][1] give the
    specification's +-inf (in output 2 only, for the model), not inf * 0 = NaN."""
    dout, n = 33, 130
    rng = np.random.default_rng(din)
    mean, e = pca_model(rng, din, dout)
    clean = cnn_like(rng, n, din)
    x = clean.copy()
    x[5, 0] = np.inf
    x[n - 1, 3] = -np.inf
    spec = orc.pca_project(mean, e, x, False, flavour=1)
    assert np.isinf(spec[[5, n - 1]]).all() and np.isfinite(np.delete(spec, [5, n - 1], 0)).all()
    check_projection(amd, orc, mean, e, x, "din=%d, infinite x in columns 0 and 3" % din)
    e2 = e.copy()
    e2[2, 1] = np.inf
    spec = orc.pca_project(mean, e2, clean, False, flavour=1)
    assert np.isinf(spec[:, 2]).all() and np.isfinite(np.delete(spec, 2, 1)).all()
    check_projection(amd, orc, mean, e2, clean, "din=%d, E[2][1] = +inf" % din)


@pytest.mark.parametrize("din,dout", [(100, 33), (64, 32)])
def test_pca_magnitudes(amd, orc, din, dout):
    """rows (and mean) scaled by 1e-25: the norm is under the 1e-12 clamp and the quotients take div_rn's guarded path; scaled by
    1e15: a divisor above its fast range; a row equal to the mean: all +0.0 under both epilogues; -0.0 inputs"""
    n = 129
    rng = np.random.default_rng(din * 7 + dout)
    mean, e = pca_model(rng, din, dout)
    x = cnn_like(rng, n, din)
    for scale in (1e-25, 1e15):
        s = F32(scale)
        out = check_projection(amd, orc, mean * s, e, x * s, "%d -> %d, scale %g" % (din, dout, scale))
        norms = np.linalg.norm(out[False].astype(np.float64), axis=1)
        assert (norms < 1e-12).all() if scale < 1 else (norms > 2.0 ** 40).all()
    xm = x.copy()
    xm[0] = mean; xm[64] = mean; xm[n - 1] = mean
    out = check_projection(amd, orc, mean, e, xm, "%d -> %d, rows equal to the mean" % (din, dout))
    for l2 in (False, True):
        assert (bits(out[l2][[0, 64, n - 1]]) == 0).all()
    xz = x.copy()
    xz[3] = -0.0
    xz[:, 0:din:5][xz[:, 0:din:5] == 0] = -0.0
    assert np.signbit(xz).sum() > din
    check_projection(amd, orc, mean, e, xz, "%d -> %d, -0.0 inputs" % (din, dout))
    check_projection(amd, orc, np.zeros(din, F32), e, xz, "%d -> %d, -0.0 inputs, zero mean" % (din, dout))
