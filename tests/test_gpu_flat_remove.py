"""GPU: cvtmi_flat_remove_labels (csrc/flat_remove.hip) and the layers above it.

Two oracles, no tolerance anywhere:
  numpy on the rows and the labels the searches report   kept mask, remap, removed, the labels of the kept rows;
  a FRESH handle given only the kept rows and labels      every search answers bit for bit as it does (the contract of the header).
One case per row layout is also compared against the CPU oracle's flat_search over the kept rows.

Shapes: n around the 64-lane wave, the 64-row block of the fp32 layout and the 256-row tile; fp32 at D = 4, 32, 128 (blocked) and 37
(row-major, a row of 148 bytes), uint8 at D = 32 (norms, 16-byte units), 48 (no norms) and 5 (single bytes); "remove_chunk" = 256 puts
5 chunk seams into 1025 rows.  The derived copies are tested on the smallest tables each route takes (cvtmi_flat_describe_dispatch)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IP, L2F, L2U8 = 0, 1, 2
NS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
LAYOUTS = [(IP, 4), (IP, 32), (IP, 128), (IP, 37), (L2F, 4), (L2F, 32), (L2F, 128), (L2F, 37), (L2U8, 32), (L2U8, 48), (L2U8, 5)]
LABEL_MODES = ["implicit", "implicit_base", "explicit", "explicit_x3"]
BASE = 10 ** 10
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
K, NQ = 10, 5


@pytest.fixture(scope="module")
def amd():
    import torch
    torch.cuda.is_available()
    import cvt_amd
    return cvt_amd


def make_rows(metric, n, D, seed):
    """rows with exact duplicates in them: (distance, row) ties on both sides of whatever is removed"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(n, D), dtype=np.uint8) if metric == L2U8 else rng.normal(size=(n, D)).astype(np.float32)
    for j in range(3, n, 7):
        x[j] = x[j % 3]
    return x


def make_queries(metric, D, seed, nq=NQ, rows=None):
    rng = np.random.default_rng(seed + 77)
    q = rng.integers(0, 256, size=(nq, D), dtype=np.uint8) if metric == L2U8 else rng.normal(size=(nq, D)).astype(np.float32)
    if rows is not None and len(rows):
        q[0] = rows[0]   # the duplicated row itself: its copies tie at distance 0
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


def build(amd, metric, D, rows, labels=None, base=0, chunk=0):
    ix = amd.FlatIndex(metric, D)
    if base:
        ix.set_id_base(base)
    if chunk:
        ix.set_param("remove_chunk", chunk)
    if len(rows):
        ix.add(rows, labels)
    return ix


def same_answers(a, b, q, k, what):
    da, ia = a.search(q, k)
    db, ib = b.search(q, k)
    assert np.array_equal(ia, ib), what
    assert np.array_equal(np.ascontiguousarray(da).view(np.uint32), np.ascontiguousarray(db).view(np.uint32)), what
    return da, ia


def expected(reported, rmset):
    keep = ~np.isin(reported, np.asarray(rmset, dtype=np.int64))
    remap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)
    return keep, remap


def remove_and_check(amd, ix, metric, D, rows, reported, rmset, q, what, dev=False):
    """one removal on ix (which holds `rows` reporting `reported`): counts, remap and the answers of a fresh handle over the kept rows"""
    keep, remap_e = expected(reported, rmset)
    rmset = np.ascontiguousarray(rmset, dtype=np.int64)
    if dev:
        import torch
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            removed, remap = ix.remove_labels(torch.from_numpy(rmset).cuda(), want_remap=True)
        s.synchronize()
        remap = remap.cpu().numpy()
    else:
        removed, remap = ix.remove_labels(rmset, want_remap=True)
    assert removed == int((~keep).sum()), what
    assert np.array_equal(remap, remap_e), what
    assert ix.ntotal == int(keep.sum()), what
    rows_k, lab_k = rows[keep], reported[keep]
    if len(rows_k):
        fresh = build(amd, metric, D, rows_k, lab_k)
        if dev:
            import torch
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                qd = torch.from_numpy(q).cuda()
                d1, i1 = ix.search(qd, K)
                d2, i2 = fresh.search(qd, K)
            s.synchronize()
            assert torch.equal(i1, i2) and torch.equal(d1.view(torch.int32), d2.view(torch.int32)), what
        same_answers(ix, fresh, q, K, what)
        fresh.close()
    return rows_k, lab_k


# ---- 1. every layout at the row counts around wave, block and tile; label modes and entries rotate through the grid ----
@pytest.mark.parametrize("metric,D", LAYOUTS)
def test_shapes(amd, metric, D):
    turn = 0
    for n in NS:
        rows = make_rows(metric, n, D, seed=n + D)
        q = make_queries(metric, D, n, rows=rows)
        for chunk in ([0, 256] if n > 256 else [0]):
            mode = LABEL_MODES[turn % 4]
            dev = turn % 3 == 2
            turn += 1
            labels, base, reported = make_labels(mode, n, seed=n)
            rng = np.random.default_rng(turn)
            rmset = reported[rng.random(n) < 0.3]
            what = (metric, D, n, chunk, mode, dev)
            ix = build(amd, metric, D, rows, labels, base, chunk)
            remove_and_check(amd, ix, metric, D, rows, reported, rng.permutation(rmset), q, what, dev=dev)
            ix.close()


# ---- 2. / 3. / 4. the removal sets, on every label mode ----
def removal_sets(reported, rng):
    n = len(reported)
    absent = np.array([I64_MIN + 1, I64_MAX - 1, -7 - 2 ** 40, 2 ** 62, BASE - 1, BASE + n, n, -1], dtype=np.int64)
    absent = absent[~np.isin(absent, reported)]
    r30 = reported[rng.random(n) < 0.3]
    return {
        "random30": r30,
        "first": reported[:1],
        "last": reported[-1:],
        "block": reported[64:128],
        "tile": reported[256:512],
        "all_but_one": np.delete(reported, n // 2),
        "dups_shuffled": rng.permutation(np.concatenate([r30, r30, r30[:7], absent])),
        "extremes": np.concatenate([absent, reported[n // 2:n // 2 + 1], reported[-1:]]),   # explicit modes: I64_MIN and I64_MAX are labels
    }


@pytest.mark.parametrize("mode", LABEL_MODES)
@pytest.mark.parametrize("metric,D", [(L2F, 32), (IP, 37), (L2U8, 32), (L2U8, 5)])
def test_sets(amd, metric, D, mode):
    n = 1025
    rows = make_rows(metric, n, D, seed=3 * D)
    q = make_queries(metric, D, 9, rows=rows)
    labels, base, reported = make_labels(mode, n, seed=11)
    for name, rmset in removal_sets(reported, np.random.default_rng(D)).items():
        ix = build(amd, metric, D, rows, labels, base, chunk=256)
        remove_and_check(amd, ix, metric, D, rows, reported, rmset, q, (metric, D, mode, name), dev=name in ("block", "extremes"))
        ix.close()


@pytest.mark.parametrize("metric,D", [(L2F, 32), (IP, 37), (L2U8, 32)])
def test_nothing_dropped_leaves_the_handle_alone(amd, metric, D):
    n = 1025
    rows = make_rows(metric, n, D, seed=D)
    q = make_queries(metric, D, 2, rows=rows)
    ix = build(amd, metric, D, rows, None, BASE)
    before = ix.search(q, K)
    for rmset in (np.array([BASE - 1, BASE + n, 0, n - 1, I64_MIN, I64_MAX, -BASE], dtype=np.int64), np.zeros(0, np.int64)):
        removed, remap = ix.remove_labels(rmset, want_remap=True)
        assert removed == 0 and np.array_equal(remap, np.arange(n)) and ix.ntotal == n
    after = ix.search(q, K)
    assert np.array_equal(before[1], after[1]) and np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32))
    assert after[1].min() >= BASE                      # still implicit: id_base + row ...
    ix.set_id_base(BASE + 5)                           # ... which follows id_base, as no label array does
    assert np.array_equal(ix.search(q, K)[1], after[1] + 5)
    ix.close()


@pytest.mark.parametrize("metric,D", [(L2F, 32), (IP, 37), (L2U8, 32), (L2U8, 48)])
def test_everything_then_add_again(amd, metric, D):
    n = 300
    rows = make_rows(metric, n, D, seed=D)
    q = make_queries(metric, D, 4, rows=rows)
    ix = build(amd, metric, D, rows, None, 0, chunk=256)
    removed, remap = ix.remove_labels(np.arange(n)[::-1], want_remap=True)
    assert removed == n and ix.ntotal == 0 and np.array_equal(remap, np.full(n, -1))
    assert ix.remove_labels(np.arange(4)) == 0         # an empty index is usable
    more = make_rows(metric, 130, D, seed=D + 1)
    lab = np.arange(130, dtype=np.int64) * 3 - 50
    ix.add(more, lab)
    fresh = build(amd, metric, D, more, lab)
    same_answers(ix, fresh, q, K, (metric, D))
    ix.add(rows[:70])                                   # without labels: numbered by position
    fresh.add(rows[:70])
    d, i = same_answers(ix, fresh, q, K, (metric, D))
    assert ix.ntotal == 200
    ix.close(); fresh.close()


# ---- 6. removal, add with labels, search, a second removal on the same handle ----
@pytest.mark.parametrize("metric,D", [(L2F, 128), (IP, 37), (L2U8, 32), (L2U8, 5)])
def test_remove_add_remove(amd, metric, D):
    n = 700
    rows = make_rows(metric, n, D, seed=D)
    q = make_queries(metric, D, 6, rows=rows)
    rng = np.random.default_rng(D)
    ix = build(amd, metric, D, rows, None, BASE, chunk=256)
    reported = BASE + np.arange(n, dtype=np.int64)
    rows, reported = remove_and_check(amd, ix, metric, D, rows, reported, reported[rng.random(n) < 0.4], q, "first")
    more = make_rows(metric, 333, D, seed=D + 9)
    lab = 5 * BASE + np.arange(333, dtype=np.int64)
    ix.add(more, lab)
    rows, reported = np.concatenate([rows, more]), np.concatenate([reported, lab])
    fresh = build(amd, metric, D, rows, reported)
    same_answers(ix, fresh, q, K, "after add")
    fresh.close()
    rows, reported = remove_and_check(amd, ix, metric, D, rows, reported, reported[rng.random(len(reported)) < 0.5], q, "second", dev=True)
    remove_and_check(amd, ix, metric, D, rows, reported, reported[:1], q, "third")
    ix.close()


# ---- the CPU oracle over the kept rows, once per layout ----
@pytest.mark.parametrize("metric,D", [(L2F, 32), (IP, 37), (L2U8, 32)])
def test_against_the_cpu_oracle(amd, orc, metric, D):
    n = 1025
    rng = np.random.default_rng(D)
    rows = rng.integers(0, 256, size=(n, D), dtype=np.uint8) if metric == L2U8 else rng.normal(size=(n, D)).astype(np.float32)
    rows[700] = rows[5]; rows[20] = rows[5]            # ties on both sides of removed rows (labels ascend: (distance, label) = (distance, row))
    q = make_queries(metric, D, 1, rows=rows[5:6])
    ix = build(amd, metric, D, rows, None, BASE, chunk=256)
    reported = BASE + np.arange(n, dtype=np.int64)
    keep, _ = expected(reported, reported[6:700:3])
    assert ix.remove_labels(reported[6:700:3]) == int((~keep).sum())
    d, i = ix.search(q, K)
    od, odi, oi = orc.flat_search(metric, rows[keep], q, K, labels=reported[keep])
    assert np.array_equal(i, oi)
    if metric == L2U8:
        assert np.array_equal(d, odi)
    else:
        assert np.array_equal(d.view(np.uint32), od.view(np.uint32))
    ix.close()


# ---- 7. / 8. the derived copies, on the smallest table every route takes ----
def dispatch(amd, metric, D, n, nq, k):
    out = (C.c_int * 4)()
    assert amd.lib().cvtmi_flat_describe_dispatch(metric, D, C.c_int64(n), C.c_int64(nq), k, out) == 0
    return list(out)


@pytest.fixture()
def low_min_rows(amd):
    keys = {"flat_f32_tfilter_min_rows": 32768, "flat_u8_tfilter_min_rows": 65536}
    old = {key: amd.get_tuning(key) for key in keys}
    for key, v in keys.items():
        amd.set_tuning(key, v)
    yield
    for key, v in old.items():
        amd.set_tuning(key, v)


ROUTES = {
    # name: (metric, D, candidate row counts, candidate batches, what describe_dispatch must say, what last_search reports)
    "f32_stream": (L2F, 32, [40000], [8], lambda o: o[0] == 1, 2),
    "f32_tfilter": (L2F, 32, [40000], [128, 256, 1000], lambda o: o[0] == 2, 3),
    "u8_tfilter": (L2U8, 32, [70000], [8, 256, 1000], lambda o: o[2] == 2, 4),
    "u8_stream": (L2U8, 128, [70000], [8], lambda o: o[2] == 0 and o[3] == 1, 0),
}


def pick_route(amd, name):
    metric, D, ns, nqs, pred, code = ROUTES[name]
    for n in ns:
        for nq in nqs:
            # the table shrinks by 5 % and by 100 rows more: the route must hold on the way
            if all(pred(dispatch(amd, metric, D, m, nq, K)) for m in (n, n - n // 20, n - n // 20 - 100)):
                return metric, D, n, nq, code
    raise AssertionError("no table of the candidates takes route " + name)


@pytest.mark.parametrize("name", list(ROUTES))
def test_derived_copies(amd, low_min_rows, name):
    metric, D, n, nq, code = pick_route(amd, name)
    rng = np.random.default_rng(n)
    rows = make_rows(metric, n, D, seed=n)
    q = make_queries(metric, D, 3, nq=nq, rows=rows)
    ix = build(amd, metric, D, rows)
    ix.search(q, K)                                        # the copies exist
    assert ix.last_search()[0] == code, name
    reported = np.arange(n, dtype=np.int64)
    drop = rng.permutation(n)[:n // 20]
    keep, _ = expected(reported, drop)
    assert ix.remove_labels(drop) == n // 20
    rows, reported = rows[keep], reported[keep]
    fresh = build(amd, metric, D, rows, reported)
    same_answers(ix, fresh, q, K, name)
    assert ix.last_search()[0] == code and fresh.last_search()[0] == code, name
    fresh.close()
    # 100 rows leave, 100 new rows come: n is what it was, and no copy made for the old rows may pass for valid
    drop = reported[rng.permutation(len(reported))[:100]]
    keep, _ = expected(reported, drop)
    assert ix.remove_labels(drop) == 100
    more = make_rows(metric, 100, D, seed=n + 1)
    lab = 10 ** 6 + np.arange(100, dtype=np.int64)
    ix.add(more, lab)
    rows, reported = np.concatenate([rows[keep], more]), np.concatenate([reported[keep], lab])
    assert ix.ntotal == n - n // 20
    fresh = build(amd, metric, D, rows, reported)
    same_answers(ix, fresh, q, K, name)
    assert ix.last_search()[0] == code and fresh.last_search()[0] == code, name
    ix.close(); fresh.close()


def test_removing_the_only_nan_row_gives_the_stream_back(amd):
    metric, D, n, nq = L2F, 32, 40000, 8
    assert dispatch(amd, metric, D, n - 1, nq, K)[0] == 1
    rows = make_rows(metric, n, D, seed=8)
    rows[12345, 7] = np.nan
    q = make_queries(metric, D, 8, nq=nq, rows=rows)
    ix = build(amd, metric, D, rows)
    ix.search(q, K)
    assert ix.last_search()[0] == 0                        # a non-finite row: the exact kernels
    assert ix.remove_labels(np.array([12345])) == 1
    keep = np.arange(n) != 12345
    fresh = build(amd, metric, D, rows[keep], np.arange(n, dtype=np.int64)[keep])
    same_answers(ix, fresh, q, K, "nan row removed")
    assert ix.last_search()[0] == 2 and fresh.last_search()[0] == 2
    ix.close(); fresh.close()


# ---- 9. the host mirror ----
def test_bruteforce_mirror_removes_on_the_device():
    exe = os.path.join(ROOT, "cvt_amd", "bin", "bf_remove_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK rebuilds=1", (r.stdout, r.stderr)
