"""The PQ encode kernels by name (cvt_amd/csrc/opq_encode.hip): pq_encode_mfma_kernel<8>, <16> and <8, PERM>, pq_encode_kernel<2 .. 32>,
pq_encode_generic_kernel and coarse_assign_kernel, picked by K, the sub-vector length, the LDS footprint, the alignment of the rows,
encode_variant and the entry point.  Every GPU call runs inside cvt_amd.launch_log() and the log must EQUAL the list a host copy of the
dispatch expects (pq_encode_model.py: name, grid, block, dynamic LDS, in order -- so no other kernel ran; the models here have fewer
than 64 coarse centroids, whose assignment is one kernel whatever the row count).  test_cases_reach_their_kernels shows without a GPU that
the cases take the kernels they are listed for and together reach every instance.

Lists and codes are compared with the oracle (orc.pq_encode) on every row, NaN rows included, with array_equal.  What the hard rows
hold, and why the duplicated codewords have a codebook pass of their own, is in pq_encode_model.py.

The permuted route (cvtmi_opq_rotate_encode on a perm model with one coarse centroid) is compared with the oracle's encode of
x[:, perm]; test_permuted_list_chain_* aim at the kernel's single-list chain, which must sum (x[perm[j]] - coarse[j])^2 in ascending j."""
import functools
import os
import re

import numpy as np
import pytest

import pq_encode_model as PM

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_MFMA = PM.MFMA8 + PM.MFMA16


def sid(shape):
    return "-".join(str(v) for v in shape)


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()
    return cvt_amd


@pytest.fixture(scope="module")
def cus(amd):
    import torch
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


# ---- shared inputs and references: computed once, never written to ----

@functools.lru_cache(maxsize=None)
def model(shape):
    coarse, books = PM.model(*shape)
    coarse.flags.writeable = False
    books.flags.writeable = False
    return coarse, books


@functools.lru_cache(maxsize=None)
def hard(shape):
    x = PM.hard_rows(shape[0], shape[1], shape[3])
    x.flags.writeable = False
    return x


@functools.lru_cache(maxsize=None)
def pass_books(shape, which):
    return PM.books_for_pass(model(shape)[1], which)


_ref = {}


def oracle_hard(orc, shape, which):
    """(lists, codes) of the hard rows of a shape under one codebook pass"""
    key = (shape, which)
    if key not in _ref:
        _ref[key] = orc.pq_encode(hard(shape), model(shape)[0], pass_books(shape, which))
    return _ref[key]


# ---- CPU: the cases against the dispatch, the model against the sources, the rows against their claims ----

def test_cases_reach_their_kernels():
    """host logic: by the copy of the dispatch every case takes the kernel it is listed for, and the cases together reach all three
    matrix-core instances (told apart by the LDS bytes and by the perm argument of the call), all five VALU steps, the generic kernel
    and coarse_assign_kernel"""
    cus, seen = 256, set()

    def route(shape, variant=0, ax=True, n=300, rot=None, entry="encode"):
        D, M, K, cK = shape
        fn = PM.rotate_encode_dev if entry == "rotate_encode" else PM.encode_dev
        args = (D, M, K, cK, rot, variant, ax, n, cus) if entry == "rotate_encode" else (D, M, K, cK, variant, ax, n, cus)
        launches, rc = fn(*args)
        if rc == PM.OK:
            inst = PM.instance(D, M, K, cK, rot, variant, ax, n, entry)
            assert launches[-1][0] == inst.split("<")[0]
            assert [r[0] for r in launches].count(launches[-1][0]) == 1
            seen.add(inst)
            seen.update(r[0] for r in launches[:-1])
            return launches, rc, inst
        return launches, rc, None

    for shape in ALL_MFMA:
        D, M, K, cK = shape
        step = D // M
        assert step == (8 if shape in PM.MFMA8 else 16)
        for n in PM.MFMA_ROWS:
            for variant in (0, 2):
                launches, rc, inst = route(shape, variant, n=n)
                assert rc == PM.OK and inst == "pq_encode_mfma_kernel<%d>" % step
                assert launches[-1] == (PM.MFMA, (min(cus, PM.blocks_for(PM.blocks_for(n, 32), 8)), 1, 1), 512, PM.encm_lds(M, step))
                assert len(launches) == (1 if cK == 1 else 2)
        launches, rc, inst = route(shape, 1, n=2000)
        assert rc == PM.OK and inst == "pq_encode_kernel<%d>" % step and launches[-1] == (PM.VALU, (2, 1, 1), 256, 0)
        assert launches[0][0] == (PM.ASSIGN_REG if D <= 128 else PM.COARSE) and len(launches) == 2
    # the LDS bytes tell step 8 from step 16 at the same M, and no two shapes of a step share them unless they share M
    assert PM.encm_lds(4, 8) != PM.encm_lds(4, 16)
    assert PM.encm_lds(9, 16) == 156_708 and PM.encm_lds(10, 16) == 174_120 and PM.encm_lds(16, 8) == 147_520
    assert PM.encm_lds(9, 16) <= PM.ENCM_LDS_LIMIT < PM.encm_lds(10, 16)
    # the wrap cases: more batches of 32 rows than 8 waves x CUs, some waves make a second pass, the last batch is ragged
    for shape in PM.WRAP:
        n = PM.wrap_n(cus)
        assert route(shape, n=n)[0][-1][1] == (cus, 1, 1)
        assert cus * 8 < PM.blocks_for(n, 32) < 2 * cus * 8 and n % 32 == 1
    # refused by the LDS rule
    for shape in PM.REFUSED:
        launches, rc, inst = route(shape, 0, n=PM.PLAIN_N)
        assert rc == PM.OK and inst == "pq_encode_kernel<16>" and [r[0] for r in launches] == [PM.COARSE, PM.VALU]
        launches, rc, _ = route(shape, 2, n=PM.PLAIN_N)
        assert rc == PM.EUNSUPPORTED and [r[0] for r in launches] == [PM.COARSE]
    # the VALU steps and the generic kernel
    for shape, step in zip(PM.VALU_CASES, (2, 4, 8, 32)):
        launches, rc, inst = route(shape, n=PM.PLAIN_N)
        assert rc == PM.OK and inst == "pq_encode_kernel<%d>" % step and launches[-1] == (PM.VALU, (2, 1, 1), 256, 0)
    for shape in PM.GENERIC_CASES:
        launches, rc, inst = route(shape, n=PM.PLAIN_N)
        assert rc == PM.OK and inst == PM.GENERIC and launches[-1] == (PM.GENERIC, (6, 1, 1), 256, 0)
    # rows 4 bytes past a 16-byte boundary
    for shape in PM.MISALIGNED:
        launches, rc, inst = route(shape, 0, ax=False)
        assert rc == PM.OK and inst.startswith("pq_encode_kernel<") and [r[0] for r in launches] == [PM.ASSIGN_REG, PM.VALU]
        assert route(shape, 2, ax=False)[1] == PM.EUNSUPPORTED
    for shape in PM.MISALIGNED_PERM:
        launches, rc, inst = route(shape, 0, ax=False, rot="perm", entry="rotate_encode")
        assert rc == PM.OK and inst == "pq_encode_mfma_kernel<8>" and [r[0] for r in launches] == [PM.PERMUTE, PM.MFMA]
    # the permuted route: one launch, the gathering instance
    for shape in PM.PERM_CASES:
        for variant in (0, 2):
            launches, rc, inst = route(shape, variant, n=hard(shape).shape[0], rot="perm", entry="rotate_encode")
            assert rc == PM.OK and inst == "pq_encode_mfma_kernel<8, PERM>" and len(launches) == 1
        launches, rc, inst = route(shape, 1, rot="perm", entry="rotate_encode")
        assert inst == "pq_encode_kernel<8>" and [r[0] for r in launches] == [PM.PERMUTE, PM.ASSIGN_REG, PM.VALU]
    # a dense rotation never gathers; a perm model with several centroids neither
    launches, rc, inst = route((128, 16, 256, 1), rot="R", entry="rotate_encode")
    assert inst == "pq_encode_mfma_kernel<8>" and [r[0] for r in launches] == [PM.ROTATE, PM.MFMA]
    launches, rc, inst = route((32, 4, 256, 3), rot="perm", entry="rotate_encode")
    assert inst == "pq_encode_mfma_kernel<8>" and [r[0] for r in launches] == [PM.PERMUTE, PM.ASSIGN_REG, PM.MFMA]
    want = {"pq_encode_mfma_kernel<8>", "pq_encode_mfma_kernel<16>", "pq_encode_mfma_kernel<8, PERM>", PM.GENERIC, PM.COARSE}
    want |= {"pq_encode_kernel<%d>" % s for s in (2, 4, 8, 16, 32)}
    assert want <= seen, sorted(want - seen)


def test_model_agrees_with_the_sources():
    """the constants the host copy uses are the ones the sources hold, and every kernel opq_encode.hip launches for the encode is
    expected by a case"""
    with open(os.path.join(ROOT, "cvt_amd", "csrc", "opq_encode.hip")) as f:
        src = f.read()

    def const(name):
        return int(re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, src).group(1))

    assert const("ENCM_THREADS") == PM.ENCM_THREADS and const("ENC_V") == PM.ENC_V and const("ENCM_MIN_ROWS") == PM.ENCM_MIN_ROWS
    assert re.search(r"encm_lds\(m\)\s*<=\s*160\s*\*\s*1024", src) and PM.ENCM_LDS_LIMIT == 160 * 1024
    assert re.search(r"\(\(size_t\)m\.M \* 256 \* m\.step \+ \(size_t\)m\.M \* 256 \+ m\.M\) \* sizeof\(float\)", src)
    assert re.search(r"kStartDist\s*=\s*4294967296\.0f", src)
    with open(os.path.join(ROOT, "cvt_amd", "csrc", "common.h")) as f:
        assert re.search(r"kBlock\s*=\s*%d\b" % PM.KB, f.read())
    launched = set(re.findall(r'\blaunch(?:_lds)?\(\s*"([A-Za-z0-9_]+)"', src)) - {"lut_kernel", "lut8_kernel"}
    assert launched == {PM.MFMA, PM.VALU, PM.GENERIC, PM.COARSE}, sorted(launched)


@pytest.mark.parametrize("shape", ALL_MFMA, ids=sid)
def test_hard_rows_hold_what_they_claim(orc, shape):
    """on the oracle's output, no GPU: every code value 0 .. 255 occurs in every sub-quantiser under the plain codebook (the decode of
    the position bits in every accumulator element, tile, centroid half and lane half) and under the duplicated one every value but 200;
    both list values occur; the big rows give code 255; rows on a codeword have exactly that residual"""
    D, M, K, cK = shape
    step = D // M
    coarse, books = model(shape)
    x = hard(shape)
    assert 2000 < x.shape[0] < 2400
    lists, codes = oracle_hard(orc, shape, "plain")
    for m in range(M):
        assert len(np.unique(codes[:, m])) == 256, (shape, m)
    assert set(np.unique(lists)) == {-1} | set(range(cK))
    groups = PM.hard_table(D, M, cK)[1]
    assert (codes[groups["big"]] == 255).mean() >= 0.3             # residuals x 3e4: most sub-vectors are farther than 2^16 from every codeword
    assert (codes[groups["nonfinite"][-1]] == 255).all() and lists[groups["nonfinite"][-1]] == -1
    assert {-1, 0} <= set(lists[groups["norm"]])                   # (with three centroids the nearest need not be the first)
    dl, dc = oracle_hard(orc, shape, "dup")
    for m in range(M):
        assert set(np.unique(dc[:, m])) == set(range(256)) - {200}, (shape, m)
    ic = oracle_hard(orc, shape, "inf")[1]
    assert not (ic == 99).any()
    # rows on codewords 40 / 41: the residual the kernels form is the codeword itself
    on40, on41 = groups["on40"], groups["on41"][:8]
    assert (x[on40] - coarse[on40 % cK] == PM.flat(books, 40)[None, :]).all() and (codes[on40] == 40).all() and (dc[on40] == 40).all()
    assert (x[on41] - coarse[on41 % cK] == PM.flat(books, 41)[None, :]).all() and (codes[on41] == 41).all()
    zero = groups["zero"]
    assert (x[zero] == coarse[zero % cK]).all()
    # the ladder: both codewords win in sub-space 0, and nothing else does
    assert set(codes[groups["ladder"], 0]) == {3, 17}


@pytest.mark.parametrize("D,M", PM.ORDER_D)
def test_order_rows_decide_by_order(orc, D, M):
    """host logic: of the 64 rows with |x|^2 just under 2^32, at least 8 fall on different sides of the start value when the fp32 sum
    runs in permuted order (the reference) and in natural order; the permuted-order sums are the oracle's"""
    perm = PM.perms(D)["random"]
    x = PM.order_rows(D)
    zero = np.zeros(D, PM.F32)
    natural, permuted = PM.chain_lists(x, zero), PM.chain_lists(np.ascontiguousarray(x[:, perm]), zero)
    assert (natural != permuted).sum() >= 8, (natural != permuted).sum()
    assert set(np.unique(permuted)) == {-1, 0}
    books = PM.model(D, M, 256, 1)[1]
    assert np.array_equal(orc.pq_encode(np.ascontiguousarray(x[:, perm]), zero[None, :], books)[0], permuted)


@pytest.mark.parametrize("shape", PM.PERM_CASES, ids=sid)
def test_centroid_rows_decide_by_order(orc, shape):
    """host logic: the two rows of centroid_rows get list 0 / -1 from the reference's sum and -1 / 0 from the natural-order sum"""
    D, M, K, cK = shape
    perm = PM.perms(D)["random"]
    coarse0, x = PM.centroid_rows(D, perm)
    y = np.ascontiguousarray(x[:, perm])
    assert PM.chain_lists(y, coarse0).tolist() == [0, -1] and PM.chain_lists(x, coarse0).tolist() == [-1, 0]
    assert orc.pq_encode(y, coarse0[None, :], model(shape)[1])[0].tolist() == [0, -1]


# ---- GPU: running a case ----

def dev(a, off=0):
    """a contiguous CUDA copy of a `off` elements into a larger allocation (the allocation itself is aligned far beyond 16 bytes)"""
    import torch
    t = torch.from_numpy(np.array(a))
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(*t.shape)
    v.copy_(t)
    return v


def al16(t):
    return t.data_ptr() % 16 == 0


def make_index(amd, shape, books, coarse=None, variant=0, **rotation):
    idx = amd.OpqIndex(model(shape)[0] if coarse is None else coarse, books, **rotation)
    idx.set_param("encode_variant", variant)
    return idx


def run(amd, idx, xt, entry="encode"):
    """one call inside the launch log -> (lists, codes, log, error code)"""
    rc = PM.OK
    lists = codes = None
    with amd.launch_log() as log:
        try:
            lists, codes = (idx.rotate_encode if entry == "rotate_encode" else idx.encode)(xt)
        except amd.CvtmiError as e:
            rc = e.code
    if rc == PM.OK:
        assert al16(codes) and al16(lists)
        lists, codes = lists.cpu().numpy(), codes.cpu().numpy()
    return lists, codes, log, rc


def check_log(shape, log, expect, tag):
    """the whole log equals the dispatch copy's list; and, as the records stand: one pq_encode* record, the last; with rows wider than
    128 floats and no fused assignment a coarse_assign_kernel record before it"""
    assert log == expect, (shape, tag, log, expect)
    enc = [r for r in log if r[0].startswith("pq_encode")]
    assert len(enc) == 1 and log[-1] == enc[0], (shape, tag, log)
    if shape[0] > 128 and not (shape[3] == 1 and enc[0][0] == PM.MFMA):
        assert [r[0] for r in log[:-1]] == [PM.COARSE], (shape, tag, log)


def check_equal(got, ref, shape, tag):
    lists, codes = got
    ol, oc = ref
    bad = np.flatnonzero((codes != oc).any(axis=1) | (lists != ol))
    assert bad.size == 0, (shape, tag, "rows", bad[:8].tolist(), codes[bad[:4]].tolist(), oc[bad[:4]].tolist(), lists[bad[:8]].tolist(), ol[bad[:8]].tolist())


def encode_case(amd, cus, shape, idx, x, ref, variant, tag, off=0):
    """x[:n] through cvtmi_opq_encode_dev: the log, the lists and the codes of every row"""
    D, M, K, cK = shape
    xt = dev(x, off)
    lists, codes, log, rc = run(amd, idx, xt)
    expect, erc = PM.encode_dev(D, M, K, cK, variant, al16(xt), x.shape[0], cus)
    assert rc == erc == PM.OK, (shape, tag, rc, erc)
    check_log(shape, log, expect, tag)
    check_equal((lists, codes), ref, shape, tag)
    return log


# ---- GPU: the cases ----

@gpu
@pytest.mark.parametrize("shape", ALL_MFMA, ids=sid)
def test_matrix_core_row_counts(amd, orc, cus, shape):
    """pq_encode_mfma_kernel<8> / <16> under variant 0 and 2 on the first 1, 31, 32, 33, 255, 256, 257 hard rows: one row (every lane
    reads the clamped row 0), one short of / on / one past a wave's 32 rows and a workgroup's 256; M = 1, M no multiple of 4 (byte-wise
    stores), M = 9 at step 16 (the largest footprint the LDS rule admits), one and three coarse centroids"""
    ol, oc = oracle_hard(orc, shape, "plain")
    for variant in (0, 2):
        idx = make_index(amd, shape, pass_books(shape, "plain"), variant=variant)
        for n in PM.MFMA_ROWS:
            log = encode_case(amd, cus, shape, idx, hard(shape)[:n], (ol[:n], oc[:n]), variant, (variant, n))
            assert log[-1][0] == PM.MFMA and log[-1][3] == PM.encm_lds(shape[1], shape[0] // shape[1])
        idx.close()


@gpu
@pytest.mark.parametrize("which", PM.PASSES)
@pytest.mark.parametrize("shape", ALL_MFMA, ids=sid)
def test_matrix_core_hard_rows(amd, orc, cus, shape, which):
    """all hard rows under each codebook pass: the matrix-core kernel (variant 0), and the VALU kernel of the same step (variant 1)"""
    ref = oracle_hard(orc, shape, which)
    for variant, name in ((0, PM.MFMA), (1, PM.VALU)):
        idx = make_index(amd, shape, pass_books(shape, which), variant=variant)
        log = encode_case(amd, cus, shape, idx, hard(shape), ref, variant, (which, variant))
        assert log[-1][0] == name
        idx.close()


@gpu
@pytest.mark.parametrize("shape", PM.WRAP, ids=sid)
def test_matrix_core_grid_wraps(amd, orc, cus, shape):
    """256 CUs + 257 rows: more batches of 32 rows than the persistent grid has waves -- some waves make a second pass and the last
    batch (one live row) falls to workgroup 0.  The rows walk the hard table; every row against the oracle"""
    n = PM.wrap_n(cus)
    x, src = PM.wrap_rows(hard(shape), n)
    ol, oc = oracle_hard(orc, shape, "plain")
    assert cus * 8 < PM.blocks_for(n, 32) < 2 * cus * 8
    idx = make_index(amd, shape, pass_books(shape, "plain"))
    log = encode_case(amd, cus, shape, idx, x, (ol[src], oc[src]), 0, "wrap")
    assert log == [(PM.MFMA, (cus, 1, 1), 512, PM.encm_lds(shape[1], shape[0] // shape[1]))]
    idx.close()


@gpu
@pytest.mark.parametrize("shape", PM.REFUSED, ids=sid)
def test_lds_rule_refuses(amd, orc, cus, shape):
    """M = 10 and M = 16 at step 16 need more LDS than the rule admits: variant 0 takes pq_encode_kernel<16> (after coarse_assign_kernel:
    rows wider than 128 floats), variant 2 fails with CVTMI_EUNSUPPORTED after the assignment and launches no encode"""
    D, M, K, cK = shape
    x = PM.plain_rows(D, M, K, cK, PM.PLAIN_N)
    coarse, books = model(shape)
    ref = orc.pq_encode(x, coarse, books)
    idx = make_index(amd, shape, books)
    log = encode_case(amd, cus, shape, idx, x, ref, 0, "variant 0")
    assert [r[0] for r in log] == [PM.COARSE, PM.VALU]
    idx.set_param("encode_variant", 2)
    _, _, log, rc = run(amd, idx, dev(x))
    expect, erc = PM.encode_dev(D, M, K, cK, 2, True, x.shape[0], cus)
    assert rc == erc == PM.EUNSUPPORTED and log == expect and [r[0] for r in log] == [PM.COARSE]
    idx.close()


@gpu
@pytest.mark.parametrize("shape", PM.VALU_CASES + PM.GENERIC_CASES, ids=sid)
def test_valu_and_generic_kernels(amd, orc, cus, shape):
    """pq_encode_kernel<2>, <4>, <8> (K = 200: not the matrix-core kernel's) and <32>, pq_encode_generic_kernel (K = 17 at step 48,
    step 5): two workgroups of the VALU kernel with a ragged second one, and 1 / 255 / 1025 rows"""
    D, M, K, cK = shape
    x = PM.plain_rows(D, M, K, cK, PM.PLAIN_N)
    coarse, books = model(shape)
    ol, oc = orc.pq_encode(x, coarse, books)
    want = PM.VALU if shape in PM.VALU_CASES else PM.GENERIC
    for variant in (0, 1):
        idx = make_index(amd, shape, books, variant=variant)
        for n in (PM.PLAIN_N, 1, 255, 1025):
            log = encode_case(amd, cus, shape, idx, x[:n], (ol[:n], oc[:n]), variant, (variant, n))
            assert log[-1][0] == want
        idx.close()


@gpu
@pytest.mark.parametrize("shape", PM.MISALIGNED, ids=sid)
def test_misaligned_rows(amd, orc, cus, shape):
    """the rows start 4 bytes past a 16-byte boundary (a view into a larger tensor): variant 0 takes the VALU kernel and gives the
    aligned call's codes, variant 2 is refused.  (The code array stays aligned: the kernels store it 16 bytes at a time.)"""
    D, M, K, cK = shape
    ref = oracle_hard(orc, shape, "plain")
    idx = make_index(amd, shape, pass_books(shape, "plain"))
    log = encode_case(amd, cus, shape, idx, hard(shape), ref, 0, "misaligned", off=1)
    assert log[-1][0] == PM.VALU
    log = encode_case(amd, cus, shape, idx, hard(shape), ref, 0, "aligned")
    assert log[-1][0] == PM.MFMA
    idx.set_param("encode_variant", 2)
    xt = dev(hard(shape), 1)
    assert xt.data_ptr() % 16 == 4
    _, _, log, rc = run(amd, idx, xt)
    expect, erc = PM.encode_dev(D, M, K, cK, 2, False, xt.shape[0], cus)
    assert rc == erc == PM.EUNSUPPORTED and log == expect
    idx.close()


def permuted_inputs(shape, kind):
    """(perm, raw rows, x[:, perm]) for the hard rows of a shape"""
    perm = PM.perms(shape[0])[kind]
    x, y = PM.unpermute(hard(shape), perm)
    if kind != "repeated":
        assert np.array_equal(y.view(np.uint32), hard(shape).view(np.uint32))
    return perm, x, y


def rotate_encode_case(amd, cus, shape, idx, x, ref, variant, tag, off=0):
    D, M, K, cK = shape
    xt = dev(x, off)
    lists, codes, log, rc = run(amd, idx, xt, "rotate_encode")
    expect, erc = PM.rotate_encode_dev(D, M, K, cK, "perm", variant, al16(xt), x.shape[0], cus)
    assert rc == erc == PM.OK, (shape, tag, rc, erc)
    check_log(shape, log, expect, tag)
    check_equal((lists, codes), ref, shape, tag)
    return log


@gpu
@pytest.mark.parametrize("shape", PM.MISALIGNED_PERM, ids=sid)
def test_misaligned_rows_on_a_perm_model(amd, orc, cus, shape):
    """rotate_encode on a perm model with misaligned rows cannot gather: permute_kernel into the handle's scratch, then the fused
    matrix-core encode -- the same lists and codes"""
    perm, x, y = permuted_inputs(shape, "random")
    ref = oracle_hard(orc, shape, "plain")
    idx = make_index(amd, shape, pass_books(shape, "plain"), perm=perm)
    log = rotate_encode_case(amd, cus, shape, idx, x, ref, 0, "misaligned", off=1)
    assert [r[0] for r in log] == [PM.PERMUTE, PM.MFMA]
    idx.close()


@gpu
@pytest.mark.parametrize("kind", ["random", "identity", "repeated"])
@pytest.mark.parametrize("shape", PM.PERM_CASES, ids=sid)
def test_permuted_route(amd, orc, cus, shape, kind):
    """pq_encode_mfma_kernel<8, PERM>: rotate_encode(x) == the oracle's encode of x[:, perm] on all hard rows under every codebook
    pass, for a random permutation, the identity and a map with repeated indices (cvtmi_opq_create only range-checks the map, the
    reference's reorder_ takes any); one record with the perm route's LDS and grid, nothing else; then the first 1 .. 257 rows"""
    D, M, K, cK = shape
    perm, x, y = permuted_inputs(shape, kind)
    coarse = model(shape)[0]
    for which in PM.PASSES:
        books = pass_books(shape, which)
        ref = oracle_hard(orc, shape, which) if kind != "repeated" else orc.pq_encode(y, coarse, books)
        for variant in (0, 2):
            idx = make_index(amd, shape, books, variant=variant, perm=perm)
            log = rotate_encode_case(amd, cus, shape, idx, x, ref, variant, (kind, which, variant))
            assert log == [(PM.MFMA, (min(cus, PM.blocks_for(PM.blocks_for(x.shape[0], 32), 8)), 1, 1), 512, PM.encm_lds(M, 8))]
            if which == "plain" and variant == 0:
                for n in PM.MFMA_ROWS:
                    rotate_encode_case(amd, cus, shape, idx, x[:n], (ref[0][:n], ref[1][:n]), variant, (kind, n))
            idx.close()


@gpu
@pytest.mark.parametrize("D,M", PM.ORDER_D)
def test_permuted_list_chain_order_rows(amd, orc, cus, D, M):
    """the 64 rows of test_order_rows_decide_by_order through the permuted route (a zero centroid): the lists are the permuted-order
    decisions"""
    shape = (D, M, 256, 1)
    perm = PM.perms(D)["random"]
    x = PM.order_rows(D)
    zero = np.zeros((1, D), PM.F32)
    books = model(shape)[1]
    ref = orc.pq_encode(np.ascontiguousarray(x[:, perm]), zero, books)
    assert np.array_equal(ref[0], PM.chain_lists(np.ascontiguousarray(x[:, perm]), zero[0]))
    idx = make_index(amd, shape, books, coarse=zero, perm=perm)
    log = rotate_encode_case(amd, cus, shape, idx, x, ref, 0, "order rows")
    assert len(log) == 1 and log[0][0] == PM.MFMA
    idx.close()


@gpu
@pytest.mark.parametrize("shape", PM.PERM_CASES, ids=sid)
def test_permuted_list_chain_centroid_rows(amd, orc, cus, shape):
    """the two rows of centroid_rows through the permuted route (coarse[0][j0] = 1e4): list 0 for the row whose reference sum is
    3.6e9, -1 for the one whose natural-order sum is"""
    D, M, K, cK = shape
    perm = PM.perms(D)["random"]
    coarse0, x = PM.centroid_rows(D, perm)
    books = model(shape)[1]
    ref = orc.pq_encode(np.ascontiguousarray(x[:, perm]), coarse0[None, :], books)
    assert ref[0].tolist() == [0, -1]
    idx = make_index(amd, shape, books, coarse=coarse0[None, :], perm=perm)
    log = rotate_encode_case(amd, cus, shape, idx, x, ref, 0, "centroid rows")
    assert len(log) == 1 and log[0][0] == PM.MFMA
    idx.close()
