"""GPU: cvtmi_opq_search_ivf_masked / cvtmi_opq_mask_videos -- the k nearest entries of the probed lists among those a bitmap of
insertion indices allows (csrc/ivf_search.hip, the MASKED instantiations and ivf_mask_order_kernel).

Every comparison is on distance BITS and ids, through host pointers (numpy) and device pointers (torch).  Expected values never come
from the call under test:

  oracle A   the composed oracle of test_gpu_opq_ivf_search.py (probe heap replayed in numpy, orc.lut / orc.adc_scan per probed list),
             filtered to the allowed insertion indices before orc.topk_pairs.
  oracle B   library equivalence: a second handle with the same entries, remove_ids on the disallowed ids with want_remap, the UNMASKED
             search_ivf on it, ids mapped back through the inverse remap.  Bit-identical by the header's "in short".
"""
import os
import subprocess
import threading

import numpy as np
import pytest

from conftest import bits
from test_gpu_opq_ivf_search import (BIN, INF, KMAX, Case, get_case, oracle_scores, padded, probe_lists, skew_case, skew_queries)

from oracle import binding as ob

pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope="module")
def amd():
    import torch
    torch.cuda.is_available()
    import cvt_amd
    return cvt_amd


# ------------------------------------------------------------------------------------------ helpers
def pack(allowed, words=None):
    """bool per insertion index -> uint64 words (bit i & 63 of word i >> 6), `words` of them (default ceil(n / 64))"""
    allowed = np.asarray(allowed, bool)
    nw = (allowed.size + 63) // 64
    buf = np.zeros(max(nw, words or 0) * 8, np.uint8)
    p = np.packbits(allowed, bitorder="little")
    buf[:p.size] = p
    w = buf.view("<u8").astype(np.uint64)
    return w if words is None else np.ascontiguousarray(w[:words])


def oracle_masked(orc, case, q_raw, nprobe, allowed, rotate=True, id_base=0):
    """oracle A: per query the (up to) KMAX smallest (score, id) pairs among the allowed entries of the probed lists"""
    q_rot = orc.reorder(case.perm, q_raw) if rotate else np.ascontiguousarray(q_raw, np.float32)
    out = []
    for f in range(q_rot.shape[0]):
        s, i = oracle_scores(orc, case, q_rot[f], nprobe)
        keep = allowed[i]
        s, i = s[keep], i[keep]
        if np.isnan(s).any():
            out.append((s, i + id_base))
        else:
            out.append(orc.topk_pairs(s, KMAX, i + id_base))
    return out


def allowed_counts(orc, case, q_raw, nprobe, allowed, rotate=True):
    """per query the number of allowed entries in its probed lists"""
    q_rot = orc.reorder(case.perm, q_raw) if rotate else np.ascontiguousarray(q_raw, np.float32)
    return [sum(int(allowed[case.list_rows(l)].sum()) for l in probe_lists(q_rot[f], case.coarse, min(nprobe, case.coarseK))) for f in range(q_rot.shape[0])]


def library_equivalent(amd, case, q, nprobe, k, allowed, rotate=True):
    """oracle B: remove the disallowed entries from a second handle, search it unmasked, map the ids back"""
    other = case.index(amd)
    n = case.lists.size
    dropped, remap = other.remove_ids(np.nonzero(~allowed)[0].astype(np.int64), want_remap=True)
    assert dropped == int((~allowed).sum())
    back = np.nonzero(remap >= 0)[0]                                      # new insertion index -> old one (the kept entries keep their order)
    assert back.size == n - dropped
    d, i = other.search_ivf(q, nprobe, k, rotate=rotate)
    other.close()
    i = np.where(i >= 0, back[np.maximum(i, 0)] if back.size else -1, -1)
    return d, i


def run_both(idx, q, nprobe, k, words, rotate=True):
    import torch
    dh, ih = idx.search_ivf_masked(q, nprobe, k, words, rotate=rotate)
    wt = torch.from_numpy(words.view(np.int64).copy()).cuda()
    dd, id_ = idx.search_ivf_masked(torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda(), nprobe, k, wt, rotate=rotate)
    torch.cuda.synchronize()
    return (dh, ih), (dd.cpu().numpy(), id_.cpu().numpy())


def check(idx, q, nprobe, k, words, exp, rotate=True, nan_rows=(), what=""):
    ed, ei = padded(exp, k)
    keep = np.ones(len(exp), bool)
    keep[list(nan_rows)] = False
    for tag, (d, i) in zip(("host", "dev"), run_both(idx, q, nprobe, k, words, rotate)):
        bad = np.nonzero(keep & ((bits(d) != bits(ed)).any(axis=1) | (i != ei).any(axis=1)))[0]
        assert bad.size == 0, "%s %s nprobe=%d k=%d: %d queries differ, first %d: got %s / %s want %s / %s" % (
            what, tag, nprobe, k, bad.size, bad[0], d[bad[0]][:6], i[bad[0]][:6], ed[bad[0]][:6], ei[bad[0]][:6])
        for f in nan_rows:                                                # NaN distances, min(k, allowed candidates) distinct allowed candidates
            cand = exp[f][1]
            m = min(k, cand.size)
            assert np.isnan(d[f, :m]).all() and np.array_equal(bits(d[f, m:]), bits(np.full(k - m, INF)))
            assert len(set(i[f, :m].tolist())) == m and set(i[f, :m].tolist()) <= set(cand.tolist()) and (i[f, m:] == -1).all()


def check_equivalent(amd, idx, case, q, nprobe, k, allowed, rotate=True, what=""):
    bd, bi = library_equivalent(amd, case, q, nprobe, k, allowed, rotate)
    for tag, (d, i) in zip(("host", "dev"), run_both(idx, q, nprobe, k, pack(allowed), rotate)):
        assert np.array_equal(bits(d), bits(bd)) and np.array_equal(i, bi), "%s %s: differs from the search over the kept entries" % (what, tag)


# ------------------------------------------------------------------------------------------ 1 word edges
EDGE_LENGTHS = [5, 0, 1, 63, 64, 65, 127, 128, 255, 256, 257, 513]       # (the leading 5 moves every later start off the word grid)


def edge_case():
    case = Case(32, 16, 256, len(EDGE_LENGTHS), seed=77)
    rng = case.rng
    case.coarse = (rng.normal(size=(case.coarseK, 32)) * 0.05).astype(np.float32)
    lists = np.repeat(np.arange(case.coarseK), EDGE_LENGTHS).astype(np.int32)
    lists = lists[rng.permutation(lists.size)]                            # insertion order is not list order
    codes = rng.integers(0, 256, size=(lists.size, 16)).astype(np.uint8)
    case.set_entries(lists, codes)
    return case


def test_word_edges(amd, orc):
    case = edge_case()
    n = case.lists.size
    off = case.list_off
    assert np.array_equal(np.diff(off), EDGE_LENGTHS)
    assert all(int(off[l]) % 64 != 0 for l in range(1, case.coarseK))     # no list of the set under test starts on a word
    nonempty = [l for l in range(case.coarseK) if off[l + 1] > off[l]]
    masks = {}
    m = np.zeros(n, bool); m[[case.csr_entry[off[l]] for l in nonempty]] = True; masks["first of each list"] = m
    m = np.zeros(n, bool); m[[case.csr_entry[off[l + 1] - 1] for l in nonempty]] = True; masks["last of each list"] = m
    pos = np.arange(n)
    m = np.zeros(n, bool); m[case.csr_entry[(pos % 64 == 63) | (pos % 64 == 0)]] = True; masks["list-order positions 63 and 0 mod 64"] = m
    m = np.zeros(n, bool); m[case.csr_entry[pos % 2 == 0]] = True; masks["alternating in list order"] = m
    masks["alternating in insertion order"] = (np.arange(n) % 2 == 1)
    m = np.zeros(n, bool); m[case.csr_entry[off[11] + 300]] = True; masks["one single entry"] = m
    idx = case.index(amd)
    rng = np.random.default_rng(3)
    q_rot = (case.coarse[np.arange(8) % case.coarseK + 2] + rng.normal(size=(8, 32)) * 0.004).astype(np.float32)
    for nq in (8, 3):                                                     # (two grids: groups of lists, one list per workgroup)
        for name, allowed in masks.items():
            for nprobe in (3, 12):
                exp = oracle_masked(orc, case, q_rot[:nq], nprobe, allowed, rotate=False)
                for k in (1, 10, 2048):
                    check(idx, q_rot[:nq], nprobe, k, pack(allowed), exp, rotate=False, what=name)
    for name in ("last of each list", "list-order positions 63 and 0 mod 64", "one single entry"):
        check_equivalent(amd, idx, case, q_rot, 12, 10, masks[name], rotate=False, what=name)
    q600 = (case.coarse[np.arange(600) % case.coarseK] + rng.normal(size=(600, 32)) * 0.004).astype(np.float32)
    allowed = masks["list-order positions 63 and 0 mod 64"]               # one workgroup per query walks all twelve lists
    check(idx, q600, 12, 10, pack(allowed), oracle_masked(orc, case, q600, 12, allowed, rotate=False), rotate=False, what="edges, rule 1")
    assert idx.last_ivf_masked()["rule"] == 1
    idx.close()


# ------------------------------------------------------------------------------------------ 2 widths, k, nprobe
def planted_inf(case, name):
    """for K < 256: a copy of the case whose codes hold bytes >= K (scores of +inf)"""
    if case.K == 256:
        return case, np.zeros(0, np.int64)
    c = Case(case.D, case.M, case.K, case.coarseK, seed=1)
    c.perm, c.books, c.coarse = case.perm, case.books, case.coarse
    codes = case.codes.copy()
    planted = np.arange(3, codes.shape[0], 11)
    codes[planted, planted % case.M] = case.K + (planted % (256 - case.K)).astype(np.uint8)
    c.set_entries(case.lists, codes)
    return c, planted


@pytest.mark.parametrize("name", ["case1", "case2", "case3", "odd"])      # M = 16 (prefetch path), 8, 4, and 2 (byte path); K = 256, 200, 17
def test_widths_k_nprobe(amd, orc, name):
    case, planted = planted_inf(get_case(orc, name), name)
    n = case.lists.size
    rng = np.random.default_rng(len(name))
    dense = rng.random(n) < 0.5
    sparse = rng.random(n) < 0.002
    if planted.size:
        dense[planted[::2]] = True
    idx = case.index(amd)
    q = case.queries(12, seed=7)
    sparse[case.list_rows(probe_lists(orc.reorder(case.perm, q)[0], case.coarse, 1)[0])] = False   # query 0, nprobe = 1: nothing allowed
    probes = [1, 3, 16] + ([case.coarseK + 5] if case.coarseK <= 128 else [])
    sizes = {k: set() for k in (1, 10, 128, 129, 2048)}
    for allowed in (dense, sparse):
        for nprobe in probes:
            exp = oracle_masked(orc, case, q, nprobe, allowed)
            for k in sizes:
                check(idx, q, nprobe, k, pack(allowed), exp, what=name)
            for k in sizes:
                sizes[k] |= {"more" if c > k else "fewer" for c in allowed_counts(orc, case, q, nprobe, allowed) if c != k}
    for k, seen in sizes.items():
        assert "fewer" in seen, (k, seen)
        assert "more" in seen or (k == 2048 and name != "case1"), (k, seen)
    if planted.size:                                                      # an allowed +inf score is a result and precedes the padding
        exp = oracle_masked(orc, case, q, case.coarseK, dense)
        ed, ei = exp[0]
        inf_at = np.nonzero(np.isinf(ed))[0]
        assert inf_at.size > 0 and ed.size < KMAX and set(ei[inf_at].tolist()) <= set(planted.tolist())
        d, i = idx.search_ivf_masked(q, min(case.coarseK, 128), KMAX, pack(dense))
        assert (i[0, :ed.size] >= 0).all() and (i[0, ed.size:] == -1).all() and np.isinf(d[0, inf_at[0]:]).all()
    check_equivalent(amd, idx, case, q, 3, 100, dense, what=name)
    idx.close()


# ------------------------------------------------------------------------------------------ 3 identity masks, mask length
def test_identity_masks(amd, orc):
    import torch
    case = get_case(orc, "case2")
    part = Case(64, 8, 256, 200, seed=3)
    part.perm, part.books, part.coarse = case.perm, case.books, case.coarse
    n = 4990                                                              # 77 full words and 62 bits
    part.set_entries(case.lists[:n], case.codes[:n])
    idx = part.index(amd)
    q = case.queries(10, seed=8)
    nw = (n + 63) // 64
    ones = np.full(nw, ~np.uint64(0), np.uint64)
    for nprobe, k in ((3, 10), (16, 129), (128, 2048)):
        d0, i0 = idx.search_ivf(q, nprobe, k)
        assert (i0[:, 0] >= 0).all()
        for d, i in run_both(idx, q, nprobe, k, ones):                    # all ones: search_ivf's lists, bit for bit
            assert np.array_equal(bits(d), bits(d0)) and np.array_equal(i, i0)
        for d, i in run_both(idx, q, nprobe, k, np.zeros(nw, np.uint64)):  # all zero: padding only
            assert (i == -1).all() and np.array_equal(bits(d), bits(np.full((10, k), INF)))
    allowed = np.random.default_rng(5).random(n) < 0.3
    exp = oracle_masked(orc, part, q, 16, allowed)
    exact = pack(allowed)
    assert exact.size == nw
    check(idx, q, 16, 100, exact, exp, what="exactly ceil(n / 64) words")
    db, ib = idx.search_ivf_masked(q, 16, 100, allowed)                  # the binding packs a bool array into the same words
    ed, ei = padded(exp, 100)
    assert np.array_equal(bits(db), bits(ed)) and np.array_equal(ib, ei)
    junk = pack(allowed, words=nw + 3)
    junk[nw - 1] |= ~np.uint64(0) << np.uint64(n % 64)                    # bits at positions >= ntotal, and whole words behind them
    junk[nw:] = ~np.uint64(0)
    check(idx, q, 16, 100, junk, exp, what="bits past ntotal")
    for short in (exact[:nw - 1], exact[:0]):
        with pytest.raises(amd.CvtmiError) as e:
            idx.search_ivf_masked(q, 16, 100, short)
        assert e.value.code == EINVAL
        with pytest.raises(amd.CvtmiError) as e:
            idx.search_ivf_masked(torch.from_numpy(q).cuda(), 16, 100, torch.zeros(short.size, dtype=torch.int64, device="cuda"))
        assert e.value.code == EINVAL
    idx.add_codes(case.codes[n:n + 3], case.lists[n:n + 3])               # 4993 entries: past the word boundary, the old mask is one word short
    with pytest.raises(amd.CvtmiError) as e:
        idx.search_ivf_masked(q, 16, 100, exact)
    assert e.value.code == EINVAL
    part.set_entries(case.lists[:n + 3], case.codes[:n + 3])
    grown = np.concatenate([allowed, [True, False, True]])
    check(idx, q, 16, 100, pack(grown), oracle_masked(orc, part, q, 16, grown), what="after the append")
    empty = amd.OpqIndex(case.coarse, case.books, perm=case.perm)         # an empty index pads everything, with any mask length
    for words in (np.zeros(1, np.uint64), ones):
        for d, i in run_both(empty, q, 3, 10, words):
            assert (i == -1).all() and np.array_equal(bits(d), bits(np.full((10, 10), INF)))
    idx.close(); empty.close()


# ------------------------------------------------------------------------------------------ 4 every grid rule
def test_grid_rules_1_2_4(amd, orc):
    case = get_case(orc, "case1")
    n = case.lists.size
    idx = case.index(amd)
    allowed = np.random.default_rng(9).random(n) < 0.1
    words = pack(allowed)
    q = case.queries(600, seed=13)
    exp = oracle_masked(orc, case, q, 3, allowed)
    for nq, rule in ((600, (1,)), (7, (2, 3))):                           # (seven queries: one list per workgroup, the longest list in pieces)
        for k in (10, 300):
            check(idx, q[:nq], 3, k, words, exp[:nq], what="grid nq=%d" % nq)
            p = idx.last_ivf_masked()
            print("masked nq=%d k=%d: %s" % (nq, k, p))
            assert p["rule"] in rule and p["mask_bytes"] >= (n + 63) // 64 * 8
    assert idx.last_ivf_masked()["G"] == 1
    idx.close()
    case2 = get_case(orc, "case2")                                        # 200 lists: nq = 2 at nprobe = 128, partial lists under a 1 MB cap
    idx = case2.index(amd)
    allowed = np.random.default_rng(10).random(case2.lists.size) < 0.5
    q = case2.queries(2, seed=14)
    exp = oracle_masked(orc, case2, q, 128, allowed)
    amd.set_tuning("ivf_part_cap_mb", 1)
    try:
        check(idx, q, 128, 2048, pack(allowed), exp, what="grid rule 4")
        p = idx.last_ivf_masked()
        assert p["rule"] == 4 and 0 < p["part_bytes"] <= 1 << 20
    finally:
        amd.set_tuning("ivf_part_cap_mb", 256)
    check(idx, q, 128, 2048, pack(allowed), exp, what="grid nprobe=128")
    assert idx.last_ivf_masked()["rule"] == 2
    idx.close()


def test_grid_rule_3_long_list(amd, orc):
    case = skew_case()
    n = case.lists.size
    idx = case.index(amd)
    q_rot = skew_queries(case, 1)                                         # one query at the 40 000-row list
    NP = 16                                                               # every list: the long one, the short ones, the empty ones
    assert probe_lists(q_rot[0], case.coarse, NP)[0] == 5
    idx.search_ivf_masked(q_rot, NP, 100, pack(np.ones(n, bool)), rotate=False)
    p = idx.last_ivf_masked()                                             # the grid does not depend on the mask: the plan of the all-ones run is every run's
    print("masked rule 3: %s" % p)
    assert p["rule"] == 3 and p["pieces"] > 1
    rpp, pieces = p["rows_per_piece"], p["pieces"]
    long_rows = case.list_rows(5)
    masks = {}
    m = np.zeros(n, bool); m[long_rows[(pieces - 1) * rpp:]] = True; masks["only the last piece"] = m
    m = np.zeros(n, bool); m[long_rows[[rpp - 1, rpp]]] = True; masks["either side of a piece boundary"] = m
    m = np.zeros(n, bool); m[long_rows[[2 * rpp - 1, 2 * rpp, 300, 40000 - 1]]] = True; masks["a few rows, most tiles empty"] = m
    assert case.list_rows(12).size == 3 and case.list_rows(0).size > 0
    m = np.zeros(n, bool); m[case.list_rows(12)] = True; m[case.list_rows(0)] = True; masks["none in the long list"] = m
    for name, allowed in masks.items():
        exp = oracle_masked(orc, case, q_rot, NP, allowed, rotate=False)
        assert exp[0][0].size == int(allowed.sum())
        for k in (1, 100, 2048):
            check(idx, q_rot, NP, k, pack(allowed), exp, rotate=False, what=name)
            assert idx.last_ivf_masked()["rule"] == 3
    q600 = skew_queries(case, 600)                                        # rule 1 over the same list: whole lists, 157 tiles, nearly all skipped
    allowed = masks["a few rows, most tiles empty"] | masks["none in the long list"]
    d, i = idx.search_ivf_masked(q600, 3, 100, pack(allowed), rotate=False)
    assert idx.last_ivf_masked()["rule"] == 1
    exp = oracle_masked(orc, case, q600[:24], 3, allowed, rotate=False)
    ed, ei = padded(exp, 100)
    assert np.array_equal(bits(d[:24]), bits(ed)) and np.array_equal(i[:24], ei)
    assert any(e[0].size for e in exp)
    idx.close()


# ------------------------------------------------------------------------------------------ 5 ties across lists
def test_ties_across_lists(amd, orc):
    """the construction of test_gpu_opq_ivf_search.test_ties_across_lists: identical rows alternating between two lists with identical centroids"""
    case = Case(64, 8, 256, 6, seed=31)
    rng = case.rng
    case.coarse = (rng.normal(size=(6, 64)) * 0.05).astype(np.float32)
    a, b, c = 1, 4, 2
    case.coarse[b] = case.coarse[a]
    row0 = rng.integers(0, 256, size=8).astype(np.uint8)
    row1 = rng.integers(0, 256, size=8).astype(np.uint8)
    lists = [np.array([a if r % 2 == 0 else b for r in range(300)], np.int32)]
    codes = [np.repeat(row0[None, :], 300, axis=0)]
    codes.append(rng.integers(0, 256, size=(400, 8)).astype(np.uint8)); lists.append(rng.choice([a, b, c], size=400).astype(np.int32))
    codes.append(np.repeat(row1[None, :], 300, axis=0)); lists.append(np.full(300, c, np.int32))
    case.set_entries(np.concatenate(lists), np.concatenate(codes))
    idx = case.index(amd)
    n = case.lists.size
    q_rot = np.stack([case.coarse[a] + np.float32(0.01), case.coarse[c] + np.float32(0.01), (case.coarse[a] + case.coarse[c]) / 2]).astype(np.float32)
    assert list(probe_lists(q_rot[0], case.coarse, 2)) == [a, b]
    without = np.ones(n, bool); without[[0, 700]] = False                 # the lowest id of each run of equal scores masked out
    thinned = np.ones(n, bool); thinned[1:300:3] = False; thinned[0] = True   # ... and allowed, among holes
    for allowed in (without, thinned, np.ones(n, bool)):
        for nprobe in (2, 3, 6):
            exp = oracle_masked(orc, case, q_rot, nprobe, allowed, rotate=False)
            ks = {1, 2, 7, 100, 128, 129, 199, 200, 298, 299, 300, 301, 1000}
            for f, (ed, ei) in enumerate(exp):                            # a k that cuts every run of equal scores in the middle
                runs = np.nonzero(np.diff(bits(ed)) == 0)[0]
                if runs.size:
                    ks.add(int(runs[runs.size // 2]) + 1)
                    assert (np.diff(ei)[runs] > 0).all()
            assert any(np.array_equal(bits(ed[k - 1:k]), bits(ed[k:k + 1])) for k in ks for ed, _ in exp if ed.size > k)
            assert all((0 in ei.tolist()) <= bool(allowed[0]) for _, ei in exp)
            for k in sorted(ks):
                check(idx, q_rot, nprobe, k, pack(allowed), exp, rotate=False, what="ties")
    idx.close()


# ------------------------------------------------------------------------------------------ 6 NaN / inf queries
def test_non_finite_queries(amd, orc):
    base = get_case(orc, "case3")
    clean = Case(32, 4, 200, 40, seed=9)
    clean.perm, clean.books, clean.coarse = base.perm, base.books, base.coarse
    clean.set_entries(base.lists[:1500], base.codes[:1500])
    idx = clean.index(amd)
    q = clean.queries(10, seed=12)
    q[4, 9] = np.inf
    q[2, 5] = np.nan
    q[7, :] = np.nan
    for frac in (0.4, 0.01):
        allowed = np.random.default_rng(int(frac * 100)).random(1500) < frac
        for nprobe, k in ((3, 10), (3, 2048), (40, 100), (40, 2048)):
            exp = oracle_masked(orc, clean, q, nprobe, allowed)
            for f in (2, 7):                                              # a NaN query probes lists 0 .. nprobe-1: its candidates are their allowed entries
                want = np.concatenate([clean.list_rows(l) for l in range(nprobe)] + [np.zeros(0, np.int64)])
                assert sorted(exp[f][1].tolist()) == sorted(want[allowed[want]].tolist()) and np.isnan(exp[f][0]).all()
            assert np.isinf(exp[4][0]).all()
            check(idx, q, nprobe, k, pack(allowed), exp, nan_rows=(2, 7), what="non-finite queries")
    idx.close()


# ------------------------------------------------------------------------------------------ 7 state changes
def test_state_changes(amd, orc):
    case = get_case(orc, "case2")
    n = case.lists.size
    q = case.queries(10, seed=8)
    part = Case(64, 8, 256, 200, seed=3)
    part.perm, part.books, part.coarse = case.perm, case.books, case.coarse
    rng = np.random.default_rng(21)
    idx = amd.OpqIndex(case.coarse, case.books, perm=case.perm)
    idx.add_codes(case.codes[:2501], case.lists[:2501])
    part.set_entries(case.lists[:2501], case.codes[:2501])
    allowed = rng.random(2501) < 0.3
    check(idx, q, 3, 100, pack(allowed), oracle_masked(orc, part, q, 3, allowed), what="first search of the handle")   # (it builds the insertion indices)
    idx.set_id_base(10 ** 9)                                              # the mask addresses the insertion index, the result reports the id
    check(idx, q, 3, 100, pack(allowed), oracle_masked(orc, part, q, 3, allowed, id_base=10 ** 9), what="id base")
    idx.set_id_base(0)
    idx.add_codes(case.codes[2501:], case.lists[2501:])                   # append, then search with a mask over all n
    part.set_entries(case.lists, case.codes)
    allowed = rng.random(n) < 0.3
    exp = oracle_masked(orc, part, q, 3, allowed)
    assert max(int(e[1].max()) for e in exp if e[1].size) >= 2501
    check(idx, q, 3, 100, pack(allowed), exp, what="after append")
    gone = np.nonzero(rng.random(n) < 0.25)[0]                            # removal: the mask is built for the NEW numbering
    dropped, remap = idx.remove_ids(gone.astype(np.int64), want_remap=True)
    keep = np.setdiff1d(np.arange(n), gone)
    assert dropped == gone.size and np.array_equal(remap[keep], np.arange(keep.size))
    part.set_entries(case.lists[keep], case.codes[keep])
    allowed = rng.random(keep.size) < 0.3
    with pytest.raises(amd.CvtmiError):                                   # one word short of the NEW count
        idx.search_ivf_masked(q, 3, 100, pack(allowed)[:(keep.size + 63) // 64 - 1])
    check(idx, q, 3, 100, pack(allowed), oracle_masked(orc, part, q, 3, allowed), what="after removal")
    idx.reset()
    for d, i in run_both(idx, q, 3, 10, np.zeros(1, np.uint64)):
        assert (i == -1).all()
    idx.add_codes(case.codes[1000:1777], case.lists[1000:1777])
    part.set_entries(case.lists[1000:1777], case.codes[1000:1777])
    allowed = rng.random(777) < 0.5
    check(idx, q, 16, 129, pack(allowed), oracle_masked(orc, part, q, 16, allowed), what="after reset")
    idx.close()


# ------------------------------------------------------------------------------------------ 8 entries outside the lists
def test_entries_outside_the_lists(amd, orc):
    base = get_case(orc, "case1")
    case = Case(128, 16, 256, 64, seed=1)
    case.perm, case.books, case.coarse = base.perm, base.books, base.coarse
    lists = base.lists[:3000].copy()
    planted = np.arange(5, 3000, 37)
    lists[planted[::2]] = -1
    lists[planted[1::2]] = 64 + (planted[1::2] % 5)
    case.set_entries(lists, base.codes[:3000])
    idx = case.index(amd)
    q = case.queries(12, seed=4)
    allowed = np.random.default_rng(2).random(3000) < 0.4
    with_them, without = allowed.copy(), allowed.copy()
    with_them[planted] = True; without[planted] = False
    exp = oracle_masked(orc, case, q, 64, without)
    for k in (10, 2048):
        for m in (with_them, without):
            check(idx, q, 64, k, pack(m), exp, what="entries outside the lists")
    only = np.zeros(3000, bool); only[planted] = True                     # nothing but them: padding
    for d, i in run_both(idx, q, 64, 10, pack(only)):
        assert (i == -1).all() and np.array_equal(bits(d), bits(np.full((12, 10), INF)))
    idx.close()


# ------------------------------------------------------------------------------------------ 9 concurrency
def test_four_threads_four_masks(amd, orc):
    case = get_case(orc, "case1")
    n = case.lists.size
    idx = case.index(amd)
    q = case.queries(64, seed=15)
    rng = np.random.default_rng(33)
    jobs = [(1, 10, rng.random(n) < 0.5), (3, 100, rng.random(n) < 0.1), (16, 300, rng.random(n) < 0.01), (64, 2048, rng.random(n) < 0.3)]
    words = [pack(m) for _, _, m in jobs]
    serial = [idx.search_ivf_masked(q, nprobe, k, w) for (nprobe, k, _), w in zip(jobs, words)]
    for (nprobe, k, m), (d, i) in zip(jobs, serial):                      # the single-threaded answers are the oracle's
        ed, ei = padded(oracle_masked(orc, case, q[:8], nprobe, m), k)
        assert np.array_equal(bits(d[:8]), bits(ed)) and np.array_equal(i[:8], ei)
    wrong, errs = [], []

    def work(j):
        try:
            for r in range(24):
                d, i = idx.search_ivf_masked(q, jobs[j][0], jobs[j][1], words[j])
                if not (np.array_equal(bits(d), bits(serial[j][0])) and np.array_equal(i, serial[j][1])):
                    wrong.append((j, r))
        except Exception as e:   # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=work, args=(j,)) for j in range(len(jobs))]
    for t in ts: t.start()
    for t in ts: t.join()
    assert not errs, errs
    assert not wrong, wrong
    idx.close()


# ------------------------------------------------------------------------------------------ 10 mask_from_videos
def test_mask_from_videos(amd, orc):
    import torch
    case = get_case(orc, "case2")
    n = 4990
    rng = np.random.default_rng(44)
    lo, hi = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    pool = np.concatenate([np.array([lo, hi, -1, -7, 0, 3], np.int64), rng.integers(-50, 50, size=40)]).astype(np.int32)
    videos = pool[rng.integers(0, pool.size, size=n)]
    videos[0], videos[1], videos[n - 1] = lo, hi, -7
    idx = amd.OpqIndex(case.coarse, case.books, perm=case.perm)
    idx.add_codes(case.codes[:n], case.lists[:n], videos)
    implicit = amd.OpqIndex(case.coarse, case.books, perm=case.perm)
    implicit.add_codes(case.codes[:n], case.lists[:n])
    nw = (n + 63) // 64
    sets = [np.array([lo, hi, -7, -7, 3, 3, 3, 12345, -99999], np.int32),   # both extremes, negatives, duplicates, foreign ids
            np.array([hi], np.int32), pool[:20][::-1].copy(), np.zeros(0, np.int32), np.array([777777], np.int32)]
    for h, vid in ((idx, videos), (implicit, np.arange(n, dtype=np.int32))):
        for s in sets + [np.array([0, 63, 64, n - 1, n, -1, 2 ** 31 - 1], np.int32), rng.integers(0, n, size=900).astype(np.int32)]:
            want = pack(np.isin(vid, s))
            got = h.mask_from_videos(s)
            assert got.dtype == np.uint64 and np.array_equal(got, want), s[:8]
            wide = h.mask_from_videos(s, words=nw + 5)                    # words behind ceil(n / 64) are zeroed, bits past n are clear
            assert np.array_equal(wide[:nw], want) and not wide[nw:].any()
            dev = h.mask_from_videos(torch.from_numpy(s).cuda(), words=nw + 5)
            torch.cuda.synchronize()
            assert np.array_equal(dev.cpu().numpy().view(np.uint64), wide)
        with pytest.raises(amd.CvtmiError) as e:
            h.mask_from_videos(sets[0], words=nw - 1)
        assert e.value.code == EINVAL
        with pytest.raises(amd.CvtmiError) as e:
            h.mask_from_videos(torch.from_numpy(sets[0]).cuda(), words=nw - 1)
        assert e.value.code == EINVAL
    assert not idx.mask_from_videos(np.zeros(0, np.int32), words=nw + 2).any()   # nv = 0 clears
    # end to end: only entries of those videos come back, and they are the oracle's
    part = Case(64, 8, 256, 200, seed=3)
    part.perm, part.books, part.coarse = case.perm, case.books, case.coarse
    part.set_entries(case.lists[:n], case.codes[:n])
    q = case.queries(10, seed=8)
    pick = np.array([lo, -7, 3, 17, 17], np.int32)
    words = idx.mask_from_videos(pick)
    exp = oracle_masked(orc, part, q, 16, np.isin(videos, pick))
    check(idx, q, 16, 100, words, exp, what="mask_from_videos end to end")
    d, i = idx.search_ivf_masked(q, 16, 100, words)
    assert (i >= 0).any() and np.isin(videos[i[i >= 0]], pick).all()
    inverted = ~words                                                     # plain word operations: everything but those videos (bits past n are ignored)
    check(idx, q, 16, 100, inverted, oracle_masked(orc, part, q, 16, ~np.isin(videos, pick)), what="inverted mask")
    idx.close(); implicit.close()


# ------------------------------------------------------------------------------------------ 11 host layers
def test_cli_videos(tmp_path, amd, orc, golden):
    """opq_search --nprobe 3 --videos FILE (IVFOPQ::SearchTopKProbeMasked underneath) returns the ABI's lists; the rows of the CLI's index
    are one video each, so a video id is a row number."""
    exe = os.path.join(BIN, "opq_search")
    assert os.path.exists(exe), "host CLIs not built: __graft_entry__.build()"
    g = golden.opq["opq_ivf"]
    model = str(tmp_path / "model.bin")
    ob.write_opq_model(model, g["coarse"], g["books"], g["perm"])
    np.ascontiguousarray(g["db"], np.float32).tofile(str(tmp_path / "db.bin"))
    np.ascontiguousarray(g["queries"], np.float32).tofile(str(tmp_path / "q.bin"))
    n = g["db"].shape[0]
    rng = np.random.default_rng(6)
    vids = np.concatenate([rng.choice(n, size=n // 3, replace=False), [n + 5, -3, 0, 0]])   # unsorted, a duplicate, two ids that name nothing
    (tmp_path / "videos.txt").write_text("".join("%d\n" % v for v in vids))
    k = 20
    r = subprocess.run([exe, model, "db.bin", "q.bin", "res.txt", "--k", str(k), "--nprobe", "3", "--videos", "videos.txt"], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = (tmp_path / "res.txt").read_text().splitlines()
    assert len(lines) == g["queries"].shape[0]
    idx = amd.OpqIndex(g["coarse"], g["books"], perm=g["perm"])
    lists, codes = idx.rotate_encode(g["db"])
    idx.add_codes(codes, lists)
    allowed = np.isin(np.arange(n), vids)
    d, i = idx.search_ivf_masked(g["queries"], 3, k, pack(allowed))
    case = Case(32, 4, 256, 16, seed=0)
    case.perm, case.books, case.coarse = g["perm"], g["books"], g["coarse"]
    case.set_entries(lists, codes)
    ed, ei = padded(oracle_masked(orc, case, g["queries"], 3, allowed), k)
    assert np.array_equal(bits(d), bits(ed)) and np.array_equal(i, ei)
    for f, line in enumerate(lines):
        head, rest = line.split(" topK: ")
        ids_s, d_s = rest.split("dists: ")
        assert int(head) == f
        assert [int(t) for t in ids_s.split()] == i[f].tolist()
        assert np.array_equal(bits(np.array([float(t) for t in d_s.split()], np.float32)), bits(d[f]))
    idx.close()
