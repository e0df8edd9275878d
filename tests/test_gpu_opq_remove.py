"""GPU: cvtmi_opq_remove_videos / cvtmi_opq_remove_ids (csrc/opq_remove.hip).

Two oracles, no tolerance anywhere:
  numpy on the insertion-ordered arrays   kept mask, remap, removed, renumbered video ids, and what cvtmi_opq_get_entries returns
                                          for the kept entries (a stable sort by list id);
  a FRESH handle given only the kept entries   every search entry answers bit for bit as it does (the contract of the header).

Shapes: n around the 64-row wave and the 256-row tile, M = 16 (rotated copy), 8 and 4 (packed rotation), 12 (padded copy, a row size
that is no power of two), coarseK 1 and 8; "remove_chunk" = 256 puts 5 chunk seams into 1025 rows."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

TILE = 256
MS = [16, 8, 4, 12]
NS = [1, 63, 64, 65, 1023, 1024, 1025]
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def amd():
    import torch
    torch.cuda.is_available()
    import cvt_amd
    return cvt_amd


_MODELS = {}


def model(M, L):
    if (M, L) not in _MODELS:
        rng = np.random.default_rng(100 * M + L)
        D = 8 * M
        _MODELS[(M, L)] = ((rng.normal(size=(L, D)) * 0.3).astype(np.float32), (rng.normal(size=(M, 256, D // M)) * 0.05).astype(np.float32))
    return _MODELS[(M, L)]


def new_index(amd, M, L, id_base=0, chunk=0):
    coarse, books = model(M, L)
    idx = amd.OpqIndex(coarse, books)
    if id_base:
        idx.set_id_base(id_base)
    if chunk:
        idx.set_param("remove_chunk", chunk)
    return idx


def data(n, M, L, seed):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, size=(n, M), dtype=np.uint8)
    lists = rng.integers(0, L, size=n).astype(np.int32) if L > 1 else None
    return codes, lists


def distinct_videos(n, seed):
    """one video id per entry, all different, negatives and both extremes among them"""
    rng = np.random.default_rng(seed)
    v = rng.choice(np.arange(-4 * n - 8, 4 * n + 8), size=n, replace=False).astype(np.int64)
    if n >= 3:
        v[n // 2] = I32_MIN
        v[n - 1] = I32_MAX
    return v.astype(np.int32)


def expected_entries(L, codes, lists, vids):
    """cvtmi_opq_get_entries over these insertion-ordered arrays"""
    n = codes.shape[0]
    l = np.zeros(n, np.int64) if lists is None else lists.astype(np.int64)
    valid = np.flatnonzero((l >= 0) & (l < L))
    order = valid[np.argsort(l[valid], kind="stable")]
    off = np.concatenate([[0], np.cumsum(np.bincount(l[valid], minlength=L))]).astype(np.int64)
    v = np.arange(n, dtype=np.int32) if vids is None else vids
    return off, v[order], codes[order]


def expected_remap(drop):
    remap = np.cumsum(~drop).astype(np.int64) - 1
    remap[drop] = -1
    return remap


def check_entries(idx, L, codes, lists, vids, ctx):
    off, vid, c = idx.get_entries()
    eo, ev, ec = expected_entries(L, codes, lists, vids)
    assert np.array_equal(off, eo), ctx
    assert np.array_equal(vid, ev), ctx
    assert np.array_equal(c, ec), ctx


def patterns(n, seed):
    """name -> mask of the entries to drop"""
    rng = np.random.default_rng(seed)
    z = np.zeros(n, bool)
    seam = TILE if n > TILE else n // 2              # a run across the first chunk seam (or the middle of a small input)
    out = {"nothing": z.copy(), "everything": ~z, "first": z.copy(), "last": z.copy(), "every_other": np.arange(n) % 2 == 0, "seam_run": z.copy(),
           "random30": rng.random(n) < 0.3}
    out["first"][0] = True
    out["last"][n - 1] = True
    out["seam_run"][max(seam - 5, 0):min(seam + 7, n)] = True
    return out


def run_pattern(idx, L, n, M, name, drop, mode, base, seed):
    """reset, add n entries, drop `drop` through remove_ids / remove_videos, check against numpy; returns (entries, remap)"""
    codes, lists = data(n, M, L, seed)
    vids = distinct_videos(n, seed + 1)
    idx.reset()
    idx.add_codes(codes, lists, vids)
    rng = np.random.default_rng(seed + 2)
    if mode == "ids":
        s = base + np.flatnonzero(drop).astype(np.int64)
        if name == "nothing" and (seed + n) % 2:
            s = np.array([base - 1, base + n, base + n + 5, -7], np.int64)           # absent ids
        removed, remap = idx.remove_ids(rng.permutation(s), want_remap=True)
    else:
        s = vids[drop]
        if name == "nothing" and (seed + n) % 2:
            s = np.setdiff1d(np.array([7 * n + 100, -7 * n - 100, 12345678], np.int32), vids)   # absent ids
        removed, remap = idx.remove_videos(rng.permutation(s), want_remap=True)
    ctx = (n, M, L, name, mode)
    assert removed == int(drop.sum()), ctx
    assert idx.ntotal == n - removed, ctx
    assert np.array_equal(remap, expected_remap(drop)), ctx
    keep = ~drop
    check_entries(idx, L, codes[keep], None if lists is None else lists[keep], vids[keep], ctx)
    return idx.get_entries(), remap


@pytest.mark.parametrize("L", [1, 8])
@pytest.mark.parametrize("M", MS)
def test_removal_patterns_against_numpy(amd, M, L):
    base = 1000
    idx = new_index(amd, M, L, id_base=base)
    seed = 0
    for n in NS:
        for name, drop in patterns(n, 50 + n).items():
            for mode in ("ids", "videos"):
                seed += 1
                run_pattern(idx, L, n, M, name, drop, mode, base, seed)
    idx.close()


@pytest.mark.parametrize("M", MS)
def test_chunk_seams(amd, M):
    """1025 rows in chunks of one tile (5 chunks; a chunk size below a tile is rounded up to one) and in one default chunk: the
    same arrays and the same remap"""
    L, n = 8, 1025
    small, tiny, whole = new_index(amd, M, L, chunk=TILE), new_index(amd, M, L, chunk=1), new_index(amd, M, L)
    seed = 1000
    for name, drop in patterns(n, 77).items():
        for mode in ("ids", "videos"):
            seed += 1                                                       # ("nothing": the empty set and absent ids in turn)
            (o1, v1, c1), r1 = run_pattern(small, L, n, M, name, drop, mode, 0, seed)
            (o2, v2, c2), r2 = run_pattern(whole, L, n, M, name, drop, mode, 0, seed)
            (o3, v3, c3), r3 = run_pattern(tiny, L, n, M, name, drop, mode, 0, seed)
            for a, b, c in ((o1, o2, o3), (v1, v2, v3), (c1, c2, c3), (r1, r2, r3)):
                assert np.array_equal(a, b) and np.array_equal(a, c), (name, mode)
    with pytest.raises(amd.CvtmiError):
        small.set_param("remove_chunk", -1)
    for ix in (small, tiny, whole):
        ix.close()


def answers(idx, L, q, k, nprobe, radius, img_num):
    """every search entry over the handle, as raw bits"""
    out = {}
    if L == 1:
        d, i = idx.search(q, k)
        out["search"] = (bits(d), i)
    d, i = idx.search_ivf(q, nprobe, k)
    out["search_ivf"] = (bits(d), i)
    lims, d, i, v = idx.range_search_ivf(q, nprobe, radius, want_video=True)
    out["range"] = (lims, bits(d), i, v)
    if img_num:
        out["query_video"] = (bits(idx.query_video(q, nprobe, img_num)),)
    out["entries"] = idx.get_entries()
    return out


def same_answers(a, b, ctx):
    assert a.keys() == b.keys()
    for key in a:
        for x, y in zip(a[key], b[key]):
            assert x.shape == y.shape and np.array_equal(x, y), (ctx, key)


def fresh(amd, M, L, codes, lists, vids, variant, id_base=0):
    idx = new_index(amd, M, L, id_base=id_base)
    idx.set_param("scan_variant", variant)
    if codes.shape[0]:
        idx.add_codes(codes, lists, vids)
    return idx


@pytest.mark.parametrize("variant", [7, 3])
@pytest.mark.parametrize("L", [1, 8])
@pytest.mark.parametrize("M", MS)
def test_stale_copies_and_append(amd, M, L, variant):
    """Searches BEFORE the removal build every derived copy (rotated / packed / padded rows: cvtmi_opq_search on coarseK = 1, under
    the default dispatch and with the M = 16 scan forced; the list-ordered copy with its insertion indices: the IVF entries on
    coarseK = 8).  After the removal, and again after appending exactly as many new entries as were dropped -- the entry count the
    copies were built for -- every call answers as a fresh handle does."""
    n, k, nq, nprobe = 1025, 10, 9, (1 if L == 1 else 3)
    rng = np.random.default_rng(7 * M + L)
    codes, lists = data(n, M, L, 300 + M + L)
    vids = (np.arange(n) // 7).astype(np.int32)                               # 147 videos
    q = (rng.normal(size=(nq, 8 * M)) * 0.3).astype(np.float32)
    idx = fresh(amd, M, L, codes, lists, vids, variant, id_base=500)
    d0, _ = idx.search_ivf(q, nprobe, k)
    radius = float(np.median(d0[np.isfinite(d0)]))
    img = int(vids.max()) + 1
    before = answers(idx, L, q, k, nprobe, radius, img)
    twin = fresh(amd, M, L, codes, lists, vids, variant, id_base=500)
    same_answers(before, answers(twin, L, q, k, nprobe, radius, img), "before")
    twin.close()
    gone = np.unique(rng.integers(0, img, size=45)).astype(np.int32)
    drop = np.isin(vids, gone)
    if L == 1:
        removed = idx.remove_ids(500 + np.flatnonzero(drop))
        kv = vids[~drop]
    else:
        removed = idx.remove_videos(gone, renumber=True)
        kv = (vids[~drop] - np.searchsorted(gone, vids[~drop])).astype(np.int32)
    assert removed == int(drop.sum()) and 0 < removed < n
    kc, kl = codes[~drop], None if lists is None else lists[~drop]
    img = int(kv.max()) + 1
    ref = fresh(amd, M, L, kc, kl, kv, variant, id_base=500)
    same_answers(answers(idx, L, q, k, nprobe, radius, img), answers(ref, L, q, k, nprobe, radius, img), "after the removal")
    # append: ids continue from the new ntotal, and the index is as large as when its copies were built
    c2, l2 = data(removed, M, L, 400 + M + L)
    v2 = (img + np.arange(removed) // 5).astype(np.int32)
    idx.add_codes(c2, l2, v2)
    ref.add_codes(c2, l2, v2)
    assert idx.ntotal == n
    img = int(v2.max()) + 1
    after = answers(idx, L, q, k, nprobe, radius, img)
    same_answers(after, answers(ref, L, q, k, nprobe, radius, img), "after the append")
    _, _, ids = idx.range_search_ivf(q[:1], L, 1e30)                              # every entry: the ids run on from the kept ones
    assert np.array_equal(np.sort(ids), 500 + np.arange(n))
    idx.close(); ref.close()


def test_video_ids_extremes_duplicates_and_renumber(amd):
    M, L, n = 16, 8, 700
    codes, lists = data(n, M, L, 11)
    rng = np.random.default_rng(12)
    pool = np.array([I32_MIN, I32_MIN + 1, -7, -1, 0, 3, 5, 1 << 20, I32_MAX - 1, I32_MAX], np.int32)
    vids = pool[rng.integers(0, pool.size, size=n)]
    messy = np.array([I32_MAX, -7, I32_MIN, -7, 99, I32_MAX, 4, -7, I32_MIN], np.int32)     # unsorted, duplicates, 99 and 4 absent
    tidy = np.unique(messy)
    drop = np.isin(vids, tidy)
    keep = ~drop
    for renumber in (False, True):
        want = vids[keep] if not renumber else (vids[keep].astype(np.int64) - np.searchsorted(tidy, vids[keep])).astype(np.int32)
        got = []
        for s in (messy, tidy):
            idx = new_index(amd, M, L, chunk=TILE)
            idx.add_codes(codes, lists, vids)
            removed, remap = idx.remove_videos(s, renumber=renumber, want_remap=True)
            assert removed == int(drop.sum()) and np.array_equal(remap, expected_remap(drop))
            check_entries(idx, L, codes[keep], lists[keep], want, (renumber, s.size))
            got.append(idx.get_entries())
            idx.close()
        for a, b in zip(*got):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("L", [1, 8])
def test_implicit_video_ids(amd, L):
    M, n = 8, 321
    codes, lists = data(n, M, L, 21)
    gone = np.array([3, 300, 10, 11, 3, 320, 4000, -2], np.int32)
    drop = np.isin(np.arange(n), gone)
    keep = ~drop
    for renumber in (False, True):
        idx = new_index(amd, M, L)
        idx.add_codes(codes, lists)
        removed, remap = idx.remove_videos(gone, renumber=renumber, want_remap=True)
        assert removed == 5 and np.array_equal(remap, expected_remap(drop))
        if renumber:   # the absent id -2 counts too: every kept id drops by one more than its position asks for
            want = (np.arange(n - removed) - 1).astype(np.int32)
            assert np.array_equal(want, (np.flatnonzero(keep) - np.searchsorted(np.unique(gone), np.flatnonzero(keep))).astype(np.int32))
        else:          # an entry keeps its old number although its insertion index changed
            want = np.flatnonzero(keep).astype(np.int32)
        check_entries(idx, L, codes[keep], None if lists is None else lists[keep], want, renumber)
        idx.close()
    # renumber = 1 over ids that are all in the index: the video ids equal the new insertion indices
    idx = new_index(amd, M, L)
    idx.add_codes(codes, lists)
    assert idx.remove_videos(np.array([0, 5, 6, 320], np.int32), renumber=True) == 4
    check_entries(idx, L, np.delete(codes, [0, 5, 6, 320], 0), None if lists is None else np.delete(lists, [0, 5, 6, 320]),
                  np.arange(n - 4, dtype=np.int32), "dense")
    idx.close()


def test_renumber_counts_absent_ids_and_large_tables(amd):
    """removed ids that are not in the index but smaller than kept ones lower them; a call that drops nothing still renumbers;
    a table of more than 1024 distinct ids (the search starts from pivots in LDS) with absent ids in between"""
    M, L, n = 12, 8, 900
    codes, lists = data(n, M, L, 31)
    vids = (10 + np.arange(n) // 4).astype(np.int32)
    idx = new_index(amd, M, L, chunk=TILE)
    idx.add_codes(codes, lists, vids)
    d0 = idx.search_ivf(np.zeros((2, 8 * M), np.float32), 3, 5)                    # (the list-ordered copy exists)
    removed, remap = idx.remove_videos(np.array([2, 5, 9], np.int32), renumber=True, want_remap=True)
    assert removed == 0 and idx.ntotal == n and np.array_equal(remap, np.arange(n))
    check_entries(idx, L, codes, lists, vids - 3, "nothing dropped, ids lowered")
    vids = vids - 3
    gone = np.array([2, 5, 12, 12, 100], np.int32)
    drop = np.isin(vids, gone)
    assert idx.remove_videos(gone, renumber=True) == int(drop.sum()) == 8
    want = (vids[~drop] - np.searchsorted(np.unique(gone), vids[~drop])).astype(np.int32)
    check_entries(idx, L, codes[~drop], lists[~drop], want, "absent ids below kept ones")
    idx.close()
    n = 5000
    codes, lists = data(n, M, L, 32)
    rng = np.random.default_rng(33)
    vids = rng.choice(np.arange(-20000, 20000), size=n, replace=False).astype(np.int32)
    gone = rng.choice(np.arange(-20000, 20000), size=3500, replace=False).astype(np.int32)      # ~1/8 of them in the index
    drop = np.isin(vids, gone)
    idx = new_index(amd, M, L)
    idx.add_codes(codes, lists, vids)
    removed, remap = idx.remove_videos(gone, renumber=True, want_remap=True)
    assert removed == int(drop.sum()) and 200 < removed < n and np.array_equal(remap, expected_remap(drop))
    want = (vids[~drop] - np.searchsorted(np.sort(gone), vids[~drop])).astype(np.int32)
    check_entries(idx, L, codes[~drop], lists[~drop], want, "large table")
    idx.close()


def test_remove_ids_on_a_row_shard(amd):
    M, L, n, base, k = 16, 1, 1025, 1000, 7
    codes, _ = data(n, M, L, 41)
    rng = np.random.default_rng(42)
    q = (rng.normal(size=(5, 8 * M)) * 0.3).astype(np.float32)
    idx = new_index(amd, M, L, id_base=base, chunk=TILE)
    idx.add_codes(codes)                                                           # implicit video ids
    idx.search(q, k)
    rows = np.array([0, 1, 64, 255, 256, 600, 1024], np.int64)
    ids = np.concatenate([base + rows, base + rows[:3], [base - 1, 0, 999, base + n, base + n + 1, -5, 2 ** 40]]).astype(np.int64)
    drop = np.zeros(n, bool)
    drop[rows] = True
    removed, remap = idx.remove_ids(rng.permutation(ids), want_remap=True)
    assert removed == rows.size and np.array_equal(remap, expected_remap(drop))
    check_entries(idx, L, codes[~drop], None, np.flatnonzero(~drop).astype(np.int32), "materialised video ids")
    ref = new_index(amd, M, L, id_base=base)
    ref.add_codes(codes[~drop], None, np.flatnonzero(~drop).astype(np.int32))
    d, i = idx.search(q, k)
    rd, ri = ref.search(q, k)
    assert np.array_equal(bits(d), bits(rd)) and np.array_equal(i, ri)
    assert i.min() >= base and i.max() < base + n - removed
    # explicit video ids are left alone, and a set of absent ids touches nothing
    vids = distinct_videos(n - removed, 43)
    idx.reset()
    idx.add_codes(codes[~drop], None, vids)
    assert idx.remove_ids(np.array([base + 3, base + 3], np.int64)) == 1
    assert idx.remove_ids(np.array([5, base + n], np.int64)) == 0
    check_entries(idx, L, np.delete(codes[~drop], 3, 0), None, np.delete(vids, 3), "explicit video ids")
    idx.close(); ref.close()


def test_hidden_entries_move_like_any_other(amd):
    """list ids -1 and coarseK: never seen by the IVF entries, but they keep their place in remap and in the arrays"""
    M, L, n, k = 16, 8, 1025, 6
    codes, lists = data(n, M, L, 51)
    rng = np.random.default_rng(52)
    lists[rng.random(n) < 0.15] = -1
    lists[rng.random(n) < 0.15] = L
    vids = (np.arange(n) // 3).astype(np.int32)
    q = (rng.normal(size=(4, 8 * M)) * 0.3).astype(np.float32)
    idx = new_index(amd, M, L, chunk=TILE)
    idx.add_codes(codes, lists, vids)
    idx.search_ivf(q, 3, k)
    drop = rng.random(n) < 0.3
    removed, remap = idx.remove_ids(np.flatnonzero(drop), want_remap=True)
    assert removed == int(drop.sum()) and np.array_equal(remap, expected_remap(drop))
    hidden = (lists < 0) | (lists >= L)
    assert (hidden & ~drop).sum() > 50 and np.array_equal(remap[hidden & ~drop], expected_remap(drop)[hidden & ~drop])
    ref = new_index(amd, M, L)
    ref.add_codes(codes[~drop], lists[~drop], vids[~drop])
    img = int(vids.max()) + 1
    same_answers(answers(idx, L, q, k, 3, 1e30, img), answers(ref, L, q, k, 3, 1e30, img), "hidden")
    seen = answers(idx, L, q, k, L, 1e30, img)["range"][2]
    assert not np.isin(seen, np.flatnonzero(hidden[~drop])).any() and seen.size > 0
    # a second removal on the compacted arrays: the hidden entries were carried along in their places
    drop2 = np.arange(n - removed) % 3 == 1
    assert idx.remove_ids(np.flatnonzero(drop2)) == int(drop2.sum())
    check_entries(idx, L, codes[~drop][~drop2], lists[~drop][~drop2], vids[~drop][~drop2], "second removal")
    idx.close(); ref.close()


def test_two_scan_levels(amd):
    """more than 2048 tiles: the second level of the offset scan has more than one sum to add up"""
    M, L, n = 4, 1, 2048 * TILE + 300
    codes, _ = data(n, M, L, 61)
    rng = np.random.default_rng(62)
    drop = rng.random(n) < 0.3
    drop[:5000] = False                                                            # leading tiles stay in place
    idx = new_index(amd, M, L)
    idx.add_codes(codes)
    removed, remap = idx.remove_ids(np.flatnonzero(drop), want_remap=True)
    assert removed == int(drop.sum()) and np.array_equal(remap, expected_remap(drop))
    check_entries(idx, L, codes[~drop], None, np.flatnonzero(~drop).astype(np.int32), "two levels")
    idx.close()


def test_device_entries_on_a_side_stream(amd):
    import torch
    M, L, n = 16, 8, 1025
    codes, lists = data(n, M, L, 71)
    vids = (np.arange(n) // 5 - 40).astype(np.int32)
    gone_v = np.array([7, -40, -3, 7, 164, 9999], np.int32)
    gone_i = np.array([0, 5, 5, 1024, 300, -1, 4096], np.int64)
    stream = torch.cuda.Stream()
    for renumber in (False, True):
        host, dev = new_index(amd, M, L, chunk=TILE), new_index(amd, M, L, chunk=TILE)
        host.add_codes(codes, lists, vids)
        with torch.cuda.stream(stream):
            dev.add_codes(torch.from_numpy(codes).cuda(), torch.from_numpy(lists).cuda(), torch.from_numpy(vids).cuda())
            r1, m1 = dev.remove_videos(torch.from_numpy(gone_v).cuda(), renumber=renumber, want_remap=True)
            r2, m2 = dev.remove_ids(torch.from_numpy(gone_i).cuda(), want_remap=True)
            empty = dev.remove_ids(torch.empty(0, dtype=torch.int64, device="cuda"))
        stream.synchronize()
        h1, hm1 = host.remove_videos(gone_v, renumber=renumber, want_remap=True)
        h2, hm2 = host.remove_ids(gone_i, want_remap=True)
        assert (r1, r2, empty) == (h1, h2, 0) and r1 == 20 and r2 == 3      # (id 1024 is past the 1005 entries left)
        assert np.array_equal(m1.cpu().numpy(), hm1) and np.array_equal(m2.cpu().numpy(), hm2)
        for a, b in zip(host.get_entries(), dev.get_entries()):
            assert np.array_equal(a, b)
        assert host.ntotal == dev.ntotal == n - 23
        host.close(); dev.close()


def test_empty_index_and_everything(amd):
    M, L = 12, 8
    idx = new_index(amd, M, L)
    removed, remap = idx.remove_videos(np.array([1, 2], np.int32), want_remap=True)
    assert removed == 0 and remap.size == 0
    codes, lists = data(65, M, L, 81)
    idx.add_codes(codes, lists)
    assert idx.remove_ids(np.arange(65)) == 65 and idx.ntotal == 0
    off, vid, c = idx.get_entries()
    assert not off.any() and vid.size == 0
    q = np.zeros((2, 8 * M), np.float32)
    d, i = idx.search_ivf(q, 3, 4)
    assert np.isinf(d).all() and (i == -1).all()
    idx.add_codes(codes, lists, np.arange(65, dtype=np.int32))                      # an empty, usable index
    check_entries(idx, L, codes, lists, np.arange(65, dtype=np.int32), "refilled")
    idx.close()


def test_remove_videos_against_reference_live(amd):
    """The reference's own Add / Query loops over the 8 kept videos alone against the device index of all 12 after
    remove_videos(renumber=1): the same entries (RefOPQ.dump) and the same per-video scores, bit for bit."""
    from oracle import binding as ob
    if not ob.ref_available():
        pytest.skip("oracle/_ref not built")
    D, M, K, L, nk = 128, 16, 256, 64, 3
    rng = np.random.default_rng(199)
    coarse = (rng.normal(size=(L, D)) * 0.08).astype(np.float32)
    books = (rng.normal(size=(M, K, D // M)) * 0.03).astype(np.float32)
    perm = rng.permutation(D).astype(np.int32)
    vids = []
    for v in range(12):
        nv = int(rng.integers(50, 201))
        c = coarse[rng.integers(0, 4 if v % 3 == 0 else L, size=nv)]               # every third video crowds 4 lists
        vids.append((c[:, np.argsort(perm)] + 0.03 * rng.normal(size=(nv, D))).astype(np.float32))
    gone = [9, 0, 4, 7]
    kept = [x for v, x in enumerate(vids) if v not in gone]
    q = np.concatenate([v[:5] for v in vids]).astype(np.float32) + (0.01 * rng.normal(size=(60, D))).astype(np.float32)
    ref = ob.RefOPQ(coarse, books, perm)
    try:
        assert ref.index(kept) == len(kept)
        rms = ref.query(q, nk, len(kept))
        r_off, r_vid, r_codes = ref.dump()
    finally:
        ref.close()
    idx = amd.OpqIndex(coarse, books, perm=perm)
    idx.set_param("remove_chunk", TILE)
    for v, x in enumerate(vids):
        lists, codes = idx.encode(idx.rotate(x))
        idx.add_codes(codes, lists, np.full(x.shape[0], v, np.int32))
    idx.query_video(q, nk, len(vids))                                              # (the list-ordered copy of all 12 exists)
    assert idx.remove_videos(np.array(gone, np.int32), renumber=True) == sum(vids[v].shape[0] for v in gone)
    off, vid, codes = idx.get_entries()
    assert np.array_equal(off, r_off) and np.array_equal(vid, r_vid) and np.array_equal(codes, r_codes)
    ms = idx.query_video(q, nk, len(kept))
    assert np.array_equal(bits(ms), bits(rms))
    assert (rms < 1.0).sum() > 60
    idx.close()
