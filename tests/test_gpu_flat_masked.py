"""GPU: cvtmi_flat_search_masked / cvtmi_flat_mask_labels (csrc/flat_masked.hip) and the layers above them.

Every comparison is exact.  Expectations never come from the code under test:
  the CPU oracle  orc.flat_search over the ALLOWED rows only, in their order, flavour 4 for IP and 8 for L2F (the choice
                  test_gpu_flat_range.py makes); uint8 takes the oracle's exact int32 distances.  While labels are implicit the
                  oracle gets the labels the rows report and its (distance, label) order IS the device's (distance, row) order; with
                  explicit labels (unsorted, one of them on three rows) it gets the rows' positions, which ascend with the rows, and the
                  positions are mapped to the reported labels afterwards -- the contract orders ties by row, not by label;
  a fresh handle  cvtmi_flat_search on a second handle that holds only the allowed rows with the labels they report.
Rows hold exact duplicates (make_rows: every seventh row copies one of the first three) and query 0 is a duplicated row, so ties cross
the mask.

Shapes: n around the 64-lane wave, the 64-row block of the fp32 layout, the 256-row count tile and the 512-entry search tile; fp32 at
D = 4, 32, 128 (blocked rows, queries in SGPRs) and 37 (row-major, queries in LDS), uint8 at D = 32, 48 (16-byte pieces) and 5 (single
bytes, tail dropped)."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IP, L2F, L2U8 = 0, 1, 2
NS = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025]
LAYOUTS = [(IP, 4), (IP, 32), (IP, 128), (IP, 37), (L2F, 4), (L2F, 32), (L2F, 128), (L2F, 37), (L2U8, 32), (L2U8, 48), (L2U8, 5)]
LABEL_MODES = ["implicit", "implicit_base", "explicit", "explicit_x3"]
NQS = [1, 5, 9]
KS = [1, 10, 128, 129]
BASE = 10 ** 10
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
PAD = 0x7f800000
CVTMI_EINVAL = -1
FORM = {(IP, 4): 1, (IP, 32): 1, (IP, 128): 1, (IP, 37): 0, (L2F, 4): 1, (L2F, 32): 1, (L2F, 128): 1, (L2F, 37): 0,
        (L2U8, 32): 3, (L2U8, 48): 3, (L2U8, 5): 2, (L2U8, 80): 3, (L2U8, 160): 3}
ONES = np.uint64(2 ** 64 - 1)


@pytest.fixture(scope="module")
def amd():
    import torch
    torch.cuda.is_available()
    import cvt_amd
    return cvt_amd


def make_rows(metric, n, D, seed):
    """rows with exact duplicates in them (test_gpu_flat_range.py's): ties on both sides of any mask"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(n, D), dtype=np.uint8) if metric == L2U8 else rng.normal(size=(n, D)).astype(np.float32)
    for j in range(3, n, 7):
        x[j] = x[j % 3]
    return x


def make_queries(metric, D, seed, nq, rows=None):
    rng = np.random.default_rng(seed + 77)
    q = rng.integers(0, 256, size=(nq, D), dtype=np.uint8) if metric == L2U8 else rng.normal(size=(nq, D)).astype(np.float32)
    if rows is not None and len(rows):
        q[0] = rows[0]   # the duplicated row itself: its copies tie (L2: at distance 0)
    return q


def make_labels(mode, n, seed):
    """(labels to add with or None, id_base, the labels the searches report)"""
    if mode == "implicit":
        return None, 0, np.arange(n, dtype=np.int64)
    if mode == "implicit_base":
        return None, BASE, BASE + np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(seed + 5)
    lab = rng.choice(np.arange(-4 * n - 8, 4 * n + 8), size=n, replace=False).astype(np.int64)   # unsorted, negatives among them
    lab[::5] += 2 ** 33                                                                            # ... and labels >= 2^32
    if n >= 3:
        lab[n // 2] = I64_MIN
        lab[n - 1] = I64_MAX
    if mode == "explicit_x3" and n >= 9:
        lab[n // 3] = lab[2 * n // 3] = lab[1]   # one label on three rows
    return lab, 0, lab.copy()


def build(amd, metric, D, rows, labels=None, base=0, parts=0):
    ix = amd.FlatIndex(metric, D)
    if base:
        ix.set_id_base(base)
    if parts:
        ix.set_param("masked_parts", parts)
    if len(rows):
        ix.add(rows, labels)
    return ix


def pack(allowed, extra_words=0, fill=0):
    """bool [n] -> uint64 words, bit r & 63 of word r >> 6 = row r; `fill` goes into every bit past n"""
    n = len(allowed)
    bits = np.full(((n + 63) // 64 + extra_words) * 64, bool(fill))
    bits[:n] = allowed
    return np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def expect(orc, metric, rows, q, k, allowed, reported, mode):
    """(distance bits [nq][k] uint32, labels [nq][k]) from the CPU oracle over the allowed rows"""
    nq = len(q)
    bits = np.full((nq, k), PAD, np.uint32)
    labels = np.full((nq, k), -1, np.int64)
    idx = np.flatnonzero(allowed)
    if not len(idx):
        return bits, labels
    flavour = 4 if metric == IP else 8
    if mode.startswith("implicit"):
        od, odi, oi = orc.flat_search(metric, rows[idx], q, k, labels=reported[idx], flavour=flavour)
    else:
        od, odi, pos = orc.flat_search(metric, rows[idx], q, k, flavour=flavour)   # labels = positions in the allowed rows
        oi = np.where(pos >= 0, reported[idx][np.maximum(pos, 0)], -1)
    m = min(k, len(idx))
    assert (oi[:, m:] == -1).all()
    bits[:, :m] = u32(odi if metric == L2U8 else od)[:, :m]
    labels[:, :m] = oi[:, :m]
    return bits, labels


def run(ix, q, k, mask, dev=False):
    if not dev:
        return ix.search_masked(q, k, mask)
    import torch
    s = torch.cuda.Stream()
    words = mask if mask.dtype == np.uint64 else pack(mask)
    with torch.cuda.stream(s):
        d, i = ix.search_masked(torch.from_numpy(q).cuda(), k, torch.from_numpy(words.view(np.int64)).cuda())
    s.synchronize()            # the one wait
    return d.cpu().numpy(), i.cpu().numpy()


def check(ix, orc, metric, rows, q, k, allowed, reported, mode, what, mask=None, dev=False, fresh=None):
    eb, el = expect(orc, metric, rows, q, k, allowed, reported, mode)
    d, i = run(ix, q, k, allowed if mask is None else mask, dev)
    assert d.dtype == (np.int32 if metric == L2U8 else np.float32) and d.shape == eb.shape, what
    assert np.array_equal(u32(d), eb), what
    assert np.array_equal(i, el), what
    if fresh is not None:   # the second, independent check: the plain search of a handle that holds only the allowed rows
        if allowed.any():
            fd, fi = fresh.search(q, k)
            assert np.array_equal(u32(d), u32(fd)) and np.array_equal(i, fi), what
        else:
            assert (i == -1).all() and (u32(d) == PAD).all(), what
    return d, i


def fresh_of(amd, metric, D, rows, allowed, reported):
    if not allowed.any():
        return None
    return build(amd, metric, D, rows[allowed], reported[allowed])


def masks_of(n, seed):
    """(name, allowed bool [n], the mask as it is passed: None = the bool array itself, else uint64 words)"""
    rng = np.random.default_rng(seed)
    every = np.ones(n, bool)
    out = [("all ones", every, None), ("all zero", np.zeros(n, bool), None)]
    one = np.zeros(n, bool); one[0] = True
    out.append(("only row 0", one, pack(one)))
    one = np.zeros(n, bool); one[n - 1] = True
    out.append(("only row n-1", one, None))
    out.append(("every other row", np.arange(n) % 2 == 1, None))
    if n > 128:
        a = every.copy(); a[64:128] = False
        out.append(("one 64-row word cleared inside a tile", a, pack(a)))
    if n > 1024:
        a = every.copy(); a[512:1024] = False
        out.append(("a whole 512-row tile cleared between two populated ones", a, None))
    for p in (0.01, 0.5, 0.99):
        a = rng.random(n) < p
        out.append(("random %g" % p, a, pack(a, extra_words=1, fill=1) if p == 0.5 else None))
    out.append(("all-0xFF words longer than needed", every, np.full((n + 63) // 64 + 3, ONES, np.uint64)))
    a = np.zeros(n, bool); a[max(0, n - 200):] = True
    out.append(("clustered in the last tile", a, None))
    return out


# ---- 1. every layout at the row counts around wave, block and tiles, under every mask; label mode, batch, k and entry rotate ----
@pytest.mark.parametrize("metric,D", LAYOUTS)
def test_sizes_and_masks(amd, orc, metric, D):
    turn = LAYOUTS.index((metric, D))
    for n in NS:
        mode = LABEL_MODES[turn % 4]
        rows = make_rows(metric, n, D, seed=n + D)
        labels, base, reported = make_labels(mode, n, seed=n)
        ix = build(amd, metric, D, rows, labels, base)
        for name, allowed, mask in masks_of(n, seed=n + turn):
            nq = NQS[turn % 3]
            k = KS[(turn // 3) % 4]
            dev = turn % 4 == 3
            turn += 1
            q = make_queries(metric, D, n + turn, nq, rows=rows)
            what = (metric, D, n, name, nq, k, mode, dev)
            fresh = fresh_of(amd, metric, D, rows, allowed, reported)
            check(ix, orc, metric, rows, q, k, allowed, reported, mode, what, mask=mask, dev=dev, fresh=fresh)
            if fresh is not None:
                fresh.close()
            qt, parts, list_bytes, form = ix.last_masked()
            assert form == FORM[(metric, D)] and qt == (1 if k > 128 or nq < 4 else 4) and list_bytes == 4 * n and parts >= 1, (what, ix.last_masked())
        ix.close()


def test_every_batch_size_and_k_on_one_table(amd, orc):
    for metric, D in [(IP, 32), (L2F, 37), (L2U8, 48), (L2U8, 5)]:
        n = 513
        rows = make_rows(metric, n, D, seed=D)
        labels, base, reported = make_labels("explicit_x3", n, seed=3)
        ix = build(amd, metric, D, rows, labels, base)
        allowed = np.random.default_rng(D).random(n) < 0.5
        for nq in NQS:
            q = make_queries(metric, D, nq, nq, rows=rows)
            for k in KS:
                check(ix, orc, metric, rows, q, k, allowed, reported, "explicit_x3", (metric, D, nq, k), dev=(nq + k) % 2 == 0)
        ix.close()


# ---- 2. k: the largest, padding, and allowed == k, k - 1, 0 ----
@pytest.mark.parametrize("metric,D", [(L2F, 32), (IP, 37), (L2U8, 32)])
def test_largest_k_fits_and_pads(amd, orc, metric, D):
    n, nq, k = 4096, 5, 2048
    rows = make_rows(metric, n, D, seed=D + 1)
    q = make_queries(metric, D, 4, nq, rows=rows)
    reported = BASE + np.arange(n, dtype=np.int64)
    ix = build(amd, metric, D, rows, None, BASE)
    rng = np.random.default_rng(60)
    for share in (0.6, 0.4):
        allowed = rng.random(n) < share
        count = int(allowed.sum())
        assert (count > k) == (share == 0.6)
        d, i = check(ix, orc, metric, rows, q, k, allowed, reported, "implicit_base", (metric, D, share), dev=share == 0.4)
        m = min(k, count)
        assert (i[:, :m] >= 0).all() and (i[:, m:] == -1).all() and (u32(d[:, m:]) == PAD).all()
        assert ix.last_masked()[0] == 1   # k > 128: one query per workgroup
    ix.close()


@pytest.mark.parametrize("metric,D", [(L2F, 128), (IP, 37), (L2U8, 5)])
def test_allowed_equal_to_k_one_fewer_and_none(amd, orc, metric, D):
    n, nq = 513, 5
    rows = make_rows(metric, n, D, seed=D + 3)
    q = make_queries(metric, D, 2, nq, rows=rows)
    labels, base, reported = make_labels("explicit", n, seed=9)
    ix = build(amd, metric, D, rows, labels, base)
    rng = np.random.default_rng(D)
    for k in (1, 10, 129):
        for count in (k, k - 1, 0):
            allowed = np.zeros(n, bool)
            allowed[rng.choice(n, size=count, replace=False)] = True
            d, i = check(ix, orc, metric, rows, q, k, allowed, reported, "explicit", (metric, D, k, count), dev=count == k - 1)
            assert (i[:, :count] != -1).all() and (i[:, count:] == -1).all() and (u32(d[:, count:]) == PAD).all()
            assert all(len(set(i[f, :count].tolist())) == count for f in range(nq))
    ix.close()


# ---- 3. the parts divide the list: the same result from 1, 2, 5 and 1024 of them, and a clustered mask still splits ----
@pytest.mark.parametrize("metric,D", [(IP, 32), (L2F, 128), (L2F, 37), (L2U8, 48), (L2U8, 5), (L2U8, 80), (L2U8, 160)])
def test_parts_do_not_change_the_result(amd, orc, metric, D):
    n, nq = 1025, 9
    rows = make_rows(metric, n, D, seed=D + 4)
    q = make_queries(metric, D, 3, nq, rows=rows)
    reported = np.arange(n, dtype=np.int64)
    allowed = np.random.default_rng(D).random(n) < 0.9     # two list tiles: parts beyond them are empty and pad
    for k in (10, 129):
        first = None
        for parts in (1, 2, 5, 1024):
            ix = build(amd, metric, D, rows, parts=parts)
            d, i = check(ix, orc, metric, rows, q, k, allowed, reported, "implicit", (metric, D, k, parts), dev=parts == 5)
            assert ix.last_masked() == (1 if k > 128 else 4, parts, 4 * n, FORM[(metric, D)]), ix.last_masked()
            if first is None:
                first = (u32(d).copy(), i.copy())
            assert np.array_equal(u32(d), first[0]) and np.array_equal(i, first[1])
            ix.close()


def test_parts_parameter_range(amd):
    from cvt_amd.capi import CvtmiError
    ix = amd.FlatIndex(L2F, 32)
    for bad in (-1, 1025):
        with pytest.raises(CvtmiError):
            ix.set_param("masked_parts", bad)
    ix.set_param("masked_parts", 0)
    ix.close()


@pytest.mark.parametrize("metric,D", [(L2F, 32), (L2U8, 32)])
def test_clustered_mask_is_split_over_the_parts(amd, orc, metric, D):
    """every allowed row lies in the last quarter of the index: parts of the ROWS would leave three of four workgroups idle and one with
    everything; parts of the LIST give each a tile.  The result is the oracle's either way, with 1 part and with 4."""
    n, nq, k = 4096, 5, 10
    rows = make_rows(metric, n, D, seed=D + 5)
    q = make_queries(metric, D, 6, nq, rows=rows)
    reported = np.arange(n, dtype=np.int64)
    allowed = np.zeros(n, bool); allowed[3072:] = True
    allowed[3072 + 5::9] = False
    got = []
    for parts in (1, 4, 0):
        ix = build(amd, metric, D, rows, parts=parts)
        got.append(check(ix, orc, metric, rows, q, k, allowed, reported, "implicit", (metric, D, parts)))
        if parts:
            assert ix.last_masked()[1] == parts
        ix.close()
    for d, i in got[1:]:
        assert np.array_equal(u32(d), u32(got[0][0])) and np.array_equal(i, got[0][1])


# ---- 4. the mask of a label set ----
@pytest.mark.parametrize("mode", LABEL_MODES)
@pytest.mark.parametrize("metric,D", [(L2F, 32), (L2U8, 5)])
def test_mask_from_labels(amd, orc, metric, D, mode):
    import torch
    n, nq, k = 1025, 5, 10
    rows = make_rows(metric, n, D, seed=D + 6)
    q = make_queries(metric, D, 7, nq, rows=rows)
    labels, base, reported = make_labels(mode, n, seed=n)
    ix = build(amd, metric, D, rows, labels, base)
    rng = np.random.default_rng(n)
    words = (n + 63) // 64
    sets = {
        "a third": reported[rng.random(n) < 0.33],
        "with foreign labels, duplicates and the extremes": np.concatenate([reported[5:400:3], reported[5:400:6], [I64_MIN, I64_MAX, 12345678901234, -3],
                                                                              reported[1:2]]).astype(np.int64),
        "unsorted": reported[rng.permutation(n)[:300]],
        "empty": np.zeros(0, np.int64),
        "every label": reported,
        "foreign only": np.array([2 ** 40 + 1, -2 ** 40 - 1], dtype=np.int64),
    }
    for turn, (name, s) in enumerate(sets.items()):
        allowed = np.isin(reported, s)
        if name == "foreign only":
            allowed = np.isin(reported, s)
        want = pack(allowed)
        m = ix.mask_from_labels(s)
        assert m.dtype == np.uint64 and np.array_equal(m, want), (mode, name)
        long = ix.mask_from_labels(s, words=words + 3)                 # words past ntotal are cleared
        assert np.array_equal(long[:words], want) and not long[words:].any(), (mode, name)
        dm = ix.mask_from_labels(torch.from_numpy(s).cuda(), words=words + 2)
        torch.cuda.synchronize()
        dm = dm.cpu().numpy().view(np.uint64)
        assert np.array_equal(dm[:words], want) and not dm[words:].any(), (mode, name)
        if turn < 3 or name == "every label":
            check(ix, orc, metric, rows, q, k, allowed, reported, mode, (mode, name, "mask"), mask=m)
            check(ix, orc, metric, rows, q, k, ~allowed, reported, mode, (mode, name, "complement"), mask=~long, dev=turn % 2 == 1)
    from cvt_amd.capi import CvtmiError
    with pytest.raises(CvtmiError) as e:
        ix.mask_from_labels(reported[:3], words=words - 1)
    assert e.value.code == CVTMI_EINVAL
    ix.close()
    empty = amd.FlatIndex(metric, D)
    assert not empty.mask_from_labels(np.array([0, 1], np.int64), words=2).any() and empty.mask_from_labels(np.array([0], np.int64)).shape == (0,)
    empty.close()


# ---- 5. a masked search is the search after removing everything outside the mask ----
@pytest.mark.parametrize("metric,D", [(IP, 128), (L2F, 37), (L2U8, 32)])
@pytest.mark.parametrize("mode", ["implicit_base", "explicit"])
def test_equivalence_with_removal(amd, orc, metric, D, mode):
    n, nq, k = 1025, 9, 10
    rows = make_rows(metric, n, D, seed=D + 7)
    q = make_queries(metric, D, 8, nq, rows=rows)
    labels, base, reported = make_labels(mode, n, seed=n + 1)
    ix = build(amd, metric, D, rows, labels, base)
    copy = build(amd, metric, D, rows, labels, base)
    allowed = np.random.default_rng(D).random(n) < 0.3
    d, i = check(ix, orc, metric, rows, q, k, allowed, reported, mode, (metric, D, mode))
    assert copy.remove_labels(reported[~allowed]) == int((~allowed).sum())
    rd, ri = copy.search(q, k)
    assert np.array_equal(u32(d), u32(rd)) and np.array_equal(i, ri)
    ix.close(); copy.close()


# ---- 6. the mask addresses the rows there are now ----
@pytest.mark.parametrize("metric,D", [(L2F, 32), (L2U8, 48)])
def test_after_add_and_remove(amd, orc, metric, D):
    from cvt_amd.capi import CvtmiError
    n, nq, k = 512, 5, 10
    rows = make_rows(metric, n, D, seed=D + 8)
    q = make_queries(metric, D, 9, nq, rows=rows)
    reported = BASE + np.arange(n, dtype=np.int64)
    ix = build(amd, metric, D, rows, None, BASE)
    allowed = np.arange(n) % 3 == 0
    old = pack(allowed)                                     # 8 words: exactly the 512 rows
    check(ix, orc, metric, rows, q, k, allowed, reported, "implicit_base", "before", mask=old)
    more = make_rows(metric, 70, D, seed=D + 9)
    ix.add(more)
    rows, reported = np.concatenate([rows, more]), BASE + np.arange(n + 70, dtype=np.int64)
    for dev in (False, True):                               # built before the add: too short, not silently wrong
        with pytest.raises(CvtmiError) as e:
            run(ix, q, k, old, dev)
        assert e.value.code == CVTMI_EINVAL
    allowed = np.arange(n + 70) % 3 == 0
    check(ix, orc, metric, rows, q, k, allowed, reported, "implicit_base", "rebuilt")
    # a removal: the bits address the rows as the removal left them
    gone = np.zeros(n + 70, bool); gone[10:300:2] = True
    assert ix.remove_labels(reported[gone]) == int(gone.sum())
    rows, reported = rows[~gone], reported[~gone]
    allowed = np.arange(len(rows)) % 3 == 1
    check(ix, orc, metric, rows, q, k, allowed, reported, "explicit", "after removal", dev=True)      # (labels are an array now: rows, not labels, break ties)
    assert np.array_equal(ix.mask_from_labels(reported[allowed]), pack(allowed))
    ix.close()


# ---- 7. a NaN query: min(k, allowed) distinct allowed rows, all with NaN distances ----
@pytest.mark.parametrize("metric,D", [(IP, 32), (L2F, 128), (L2F, 37)])
def test_nan_query(amd, orc, metric, D):
    n, nq = 257, 5
    rows = make_rows(metric, n, D, seed=D)
    q = make_queries(metric, D, 1, nq, rows=rows)
    q[3, :] = np.nan
    ix = build(amd, metric, D, rows, None, BASE)
    reported = BASE + np.arange(n, dtype=np.int64)
    allowed = np.zeros(n, bool); allowed[np.random.default_rng(D).choice(n, size=40, replace=False)] = True
    valid = {BASE + int(r) for r in np.flatnonzero(allowed)}
    for k in (10, 43):
        d, i = ix.search_masked(q, k, allowed)
        m = min(k, len(valid))
        assert np.isnan(d[3, :m]).all() and len(set(i[3, :m].tolist())) == m and set(i[3, :m].tolist()) <= valid
        assert (i[3, m:] == -1).all() and (u32(d[3, m:]) == PAD).all()
        if m == len(valid):
            assert set(i[3, :m].tolist()) == valid
        finite = [0, 1, 2, 4]                                                   # the other queries are untouched by their neighbour
        eb, el = expect(orc, metric, rows, q[finite], k, allowed, reported, "implicit_base")
        assert np.array_equal(u32(d[finite]), eb) and np.array_equal(i[finite], el)
    ix.close()


# ---- 8. limits: too few mask words, an empty index, nq == 0 ----
def test_mask_words_too_small_empty_index_and_nothing(amd):
    import torch
    from cvt_amd.capi import _ptr, _stream
    lib = amd.lib()
    rows = make_rows(L2F, 65, 32, seed=1)
    ix = build(amd, L2F, 32, rows)
    q = make_queries(L2F, 32, 0, 2, rows=rows)
    mask = np.full(2, ONES, np.uint64)
    d = np.full((2, 3), 7.0, np.float32); i = np.full((2, 3), -7, np.int64)
    tq, tm = torch.from_numpy(q).cuda(), torch.from_numpy(mask.view(np.int64)).cuda()
    td, ti = torch.from_numpy(d).cuda(), torch.from_numpy(i).cuda()
    for words in (1, 0):                                     # 65 rows need 2 words
        assert lib.cvtmi_flat_search_masked(ix.h, _ptr(q), C.c_int64(2), C.c_int(3), _ptr(mask), C.c_int64(words), _ptr(d), _ptr(i)) == CVTMI_EINVAL
        assert lib.cvtmi_flat_search_masked_dev(ix.h, _ptr(tq), C.c_int64(2), C.c_int(3), _ptr(tm), C.c_int64(words), _ptr(td), _ptr(ti), _stream()) == CVTMI_EINVAL
    # nq == 0 does nothing
    assert lib.cvtmi_flat_search_masked(ix.h, _ptr(q), C.c_int64(0), C.c_int(3), _ptr(mask), C.c_int64(2), _ptr(d), _ptr(i)) == 0
    assert lib.cvtmi_flat_search_masked_dev(ix.h, None, C.c_int64(0), C.c_int(3), None, C.c_int64(0), None, None, _stream()) == 0
    for k in (0, 2049):
        assert lib.cvtmi_flat_search_masked(ix.h, _ptr(q), C.c_int64(2), C.c_int(k), _ptr(mask), C.c_int64(2), _ptr(d), _ptr(i)) == CVTMI_EINVAL
    torch.cuda.synchronize()
    assert (d == 7.0).all() and (i == -7).all() and (td.cpu().numpy() == 7.0).all() and (ti.cpu().numpy() == -7).all()
    ix.close()
    for metric, D in ((L2F, 32), (L2U8, 5)):                 # an empty index pads everything, whatever the mask holds
        empty = amd.FlatIndex(metric, D)
        q = make_queries(metric, D, 0, 3)
        for dev in (False, True):
            for m in (np.zeros(0, np.uint64), mask):
                if dev and not len(m):
                    continue
                d, i = run(empty, q, 6, m, dev)
                assert (i == -1).all() and (u32(d) == PAD).all()
        empty.close()


# ---- 9. the device entry on a stream of its own gives the host entry's bits ----
@pytest.mark.parametrize("metric,D", LAYOUTS)
def test_device_entry_equals_host_entry(amd, metric, D):
    n, nq = 1025, 9
    rows = make_rows(metric, n, D, seed=D + 10)
    q = make_queries(metric, D, 10, nq, rows=rows)
    labels, base, _ = make_labels("explicit_x3", n, seed=4)
    ix = build(amd, metric, D, rows, labels, base)
    allowed = np.random.default_rng(D).random(n) < 0.5
    for k in (10, 129):
        hd, hi = run(ix, q, k, allowed)
        dd, di = run(ix, q, k, allowed, dev=True)
        assert np.array_equal(u32(hd), u32(dd)) and np.array_equal(hi, di)
    ix.close()


# ---- 10. four threads search one handle under four different masks at once ----
@pytest.mark.parametrize("metric,D", [(L2F, 32), (L2U8, 32)])
def test_threads_on_one_handle(amd, orc, metric, D):
    n, nq, k = 1025, 5, 10
    rows = make_rows(metric, n, D, seed=D + 2)
    reported = np.arange(n, dtype=np.int64)
    ix = build(amd, metric, D, rows)
    rng = np.random.default_rng(D)
    jobs = []
    for t in range(4):
        q = make_queries(metric, D, 8 + t, nq, rows=rows)
        allowed = rng.random(n) < (0.1, 0.5, 0.9, 0.02)[t]
        jobs.append((q, allowed, expect(orc, metric, rows, q, k, allowed, reported, "implicit")))
    got, errors = [None] * 4, []

    def work(t):
        try:
            q, allowed, _ = jobs[t]
            res = []
            for _ in range(6):
                res.append(ix.search_masked(q, k, allowed))
                ix.search(q, k)                       # ... side by side with plain searches
            got[t] = res
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for t in range(4):
        eb, el = jobs[t][2]
        for d, i in got[t]:
            assert np.array_equal(u32(d), eb) and np.array_equal(i, el)
    ix.close()


# ---- 11. the host mirror ----
def test_bruteforce_mirror_filtered_search():
    exe = os.path.join(ROOT, "cvt_amd", "bin", "bf_masked_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.stdout, r.stderr)
