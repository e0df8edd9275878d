"""CPU: growing a saved graph with the host mirror (cvt_amd/host/hnswlib/hnswalg.h: loadIndex, resizeIndex, addPoint, saveIndex --
the hnsw_add CLI), against files the reference wrote.

  * hnsw_build of the first n0 rows of a golden graph, then hnsw_add ... host cont of the rest, is the golden file byte for byte:
    resizeIndex keeps what it holds, load + addPoint continues the insertion, and `cont` puts the level stream where the build left it.
  * without `cont` the stream restarts, as after the reference's loadIndex: the added rows get the levels of the first rows of a fresh
    build, and the file is the model's (tests/hnsw_build_model.py) over all rows with those levels.

The helpers at the end of this file (the schedule of a build followed by an add, spare capacity, an empty file) are shared with
tests/test_gpu_hnsw_add.py."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import hnsw_build_model as hm
from test_gpu_hnsw_build import CASES as GOLDEN, host_build, parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
_schedule = hm.schedule     # the model's own, whatever a test patches in


def host_add(tmp_path, index, rows, D, metric, name, labels=None, mode="host", cont=False):
    """hnsw_add: `index` (bytes of a saveIndex file) grown by `rows`; returns the bytes of the file it writes"""
    exe = os.path.join(BIN, "hnsw_add")
    assert os.path.exists(exe), "host CLIs not built: __graft_entry__.build()"
    src = tmp_path / (name + "_in.hnsw"); src.write_bytes(bytes(index))
    rf = tmp_path / (name + "_add_rows.bin"); rf.write_bytes(np.ascontiguousarray(rows, np.float32).tobytes())
    out = tmp_path / (name + "_out.hnsw")
    lab = "-"
    if labels is not None:
        lf = tmp_path / (name + "_add_labels.bin"); lf.write_bytes(np.ascontiguousarray(labels, np.uint64).tobytes())
        lab = str(lf)
    cmd = [exe, str(src), str(rf), str(D), str(out), "l2" if metric == 1 else "ip", lab, mode] + (["cont"] if cont else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(out, dtype=np.uint8)


def host_build_labelled(tmp_path, x, labels, metric, M, efc, name):
    rf = tmp_path / (name + "_rows.bin"); rf.write_bytes(np.ascontiguousarray(x, np.float32).tobytes())
    lf = tmp_path / (name + "_labels.bin"); lf.write_bytes(np.ascontiguousarray(labels, np.uint64).tobytes())
    out = tmp_path / (name + ".hnsw")
    r = subprocess.run([os.path.join(BIN, "hnsw_build"), str(rf), str(x.shape[1]), str(M), str(efc), str(out), "l2" if metric == 1 else "ip", str(lf)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(out, dtype=np.uint8)


# ---- 1. build of a prefix + add cont of the rest = the reference's file ---------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDEN)
def test_build_then_add_cont_is_the_golden_graph(tmp_path, golden, case):
    g = golden.hnsw
    blob = g[case + "_index"]
    metric, D, n, M, efc, k, ef = (int(v) for v in g[case + "_meta"])
    p = parse(blob)
    assert p["cnt"] == n and p["cap"] == n
    for n0 in (1, 33, n - 1):
        first = host_build_labelled(tmp_path, p["rows"][:n0], p["labels"][:n0], metric, M, efc, "%s_%d" % (case, n0))
        assert parse(first)["cap"] == n0
        out = host_add(tmp_path, first, p["rows"][n0:], D, metric, "%s_%d" % (case, n0), labels=p["labels"][n0:], cont=True)
        assert out.size == blob.size and np.array_equal(out, blob), (case, n0)


# ---- 2. without cont the level stream restarts ----------------------------------------------------------------------------------------
def test_add_after_load_restarts_the_level_stream(orc, tmp_path, monkeypatch):
    c = hm.CASES["C"]
    x, n0 = c["rows"](), 400
    n, D = x.shape
    first = host_build(tmp_path, x[:n0], c["metric"], c["M"], c["efc"], "first")
    out = host_add(tmp_path, first, x[n0:], D, c["metric"], "restart")
    got = parse(out)
    assert got["cnt"] == n and got["cap"] == n
    fresh = parse(first)["levels"]
    assert np.array_equal(got["levels"][:n0], fresh) and np.array_equal(got["levels"][n0:], fresh[:n - n0])
    assert np.array_equal(got["labels"], np.arange(n, dtype=np.uint64))
    monkeypatch.setattr(hm, "schedule", build_then_add_schedule(n0, 1, 1))
    want, cnt = hm.build_model(orc, x, c["metric"], c["M"], c["efc"], got["levels"], None, 1, vectorised=True)
    want = np.frombuffer(want, dtype=np.uint8)
    assert cnt["largest_batch"] == 1 and cnt["batches"] == n
    assert out.size == want.size and np.array_equal(out, want), hm.first_difference(got, parse(want), cnt)


# ---- shared with the GPU tests --------------------------------------------------------------------------------------------------------
def build_then_add_schedule(n0, build_batch, add_batch):
    """what hm.schedule is replaced with to model build(x[:n0], build_batch) followed by add(x[n0:], add_batch): the build's schedule
    over the first n0 rows, then the same rule restarted at row n0 -- a batch holds clamp(s // frac, 1, limit) rows and ends with the
    first row above the top level -- from the entry point and top level the build ended on.  The max_batch it is called with is
    ignored."""
    def schedule(levels, n, max_batch, frac=32, cap=8192):
        out = _schedule(levels[:n0], n0, build_batch, frac, cap)
        top, ep = int(levels[0]), 0
        for i in range(1, n0):
            if levels[i] > top:
                top, ep = int(levels[i]), i
        limit = add_batch if add_batch > 0 else cap
        s = n0
        while s < n:
            planned = min(s + min(max(1, s // frac), limit), n)
            e, cut = planned, False
            for i in range(s, planned):
                if levels[i] > top:
                    e, cut = i + 1, i + 1 < planned
                    break
            out.append((s, e, ep, top, cut))
            if levels[e - 1] > top:
                ep, top = e - 1, int(levels[e - 1])
            s = e
        return out
    return schedule


def with_capacity(blob, cap):
    """the saveIndex file `blob` with max_elements = cap >= cur_element_count: the spare level-0 blocks and level sizes are zeros"""
    blob = np.frombuffer(bytes(blob), dtype=np.uint8)
    off0, old, cnt, per, offl, offd = struct.unpack("<6Q", blob[:48].tobytes())
    assert old == cnt <= cap
    head = blob[:96].copy()
    head[8:16] = np.frombuffer(struct.pack("<Q", cap), dtype=np.uint8)
    body, tail = blob[96:96 + cnt * per], blob[96 + cnt * per:]
    return np.concatenate([head, body, np.zeros((cap - cnt) * per, np.uint8), tail, np.zeros(4 * (cap - cnt), np.uint8)])


def empty_index(D, M, efc, cap):
    """the file of HierarchicalNSW(space, cap, M, efc) before any addPoint: cur_element_count = 0, maxlevel = -1, enterpoint = -1,
    spare slots as zeros"""
    maxM0 = 2 * M
    per = 4 + 4 * maxM0 + 4 * D + 8
    head = struct.pack("<6QiI3QdQ", 0, cap, 0, per, 4 + 4 * maxM0 + 4 * D, 4 + 4 * maxM0, -1, 0xffffffff, M, maxM0, M, 1 / math.log(1.0 * M), max(efc, M))
    return np.frombuffer(head + bytes(cap * per + 4 * cap), dtype=np.uint8)


def test_helpers_agree_with_the_mirror(tmp_path, golden):
    """with_capacity and empty_index are files the mirror reads, and adding to them is adding to the file they stand for"""
    g = golden.hnsw
    blob = g["l2f7_index"]
    metric, D, n, M, efc, k, ef = (int(v) for v in g["l2f7_meta"])
    p = parse(blob)
    n0 = n - 40
    first = host_build_labelled(tmp_path, p["rows"][:n0], p["labels"][:n0], metric, M, efc, "cap")
    for cap in (n0 + 10, n):       # the rows exceed the spare capacity (resizeIndex) / fill it exactly
        out = host_add(tmp_path, with_capacity(first, cap), p["rows"][n0:], D, metric, "cap%d" % cap, labels=p["labels"][n0:], cont=True)
        assert np.array_equal(out, blob), cap
    out = host_add(tmp_path, with_capacity(first, n + 7), p["rows"][n0:], D, metric, "cap_more", labels=p["labels"][n0:], cont=True)
    assert np.array_equal(out, with_capacity(blob, n + 7))
    out = host_add(tmp_path, empty_index(D, M, efc, 5), p["rows"], D, metric, "empty", labels=p["labels"])
    assert np.array_equal(out, blob)
    schedule = build_then_add_schedule(4, 0, 0)     # a boundary forced at row 4, which the build's own schedule (frac 1) jumps over
    lv = [1, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0]
    assert _schedule(lv, 12, 0, 1, 8192)[:3] == [(1, 2, 0, 1, False), (2, 4, 0, 1, False), (4, 5, 0, 1, True)]
    assert build_then_add_schedule(3, 0, 0)(lv, 12, 0, 1, 8192) == [(1, 2, 0, 1, False), (2, 3, 0, 1, False), (3, 5, 0, 1, True),
                                                                    (5, 10, 4, 3, False), (10, 12, 4, 3, False)]
    assert schedule(lv, 12, 0, 1, 8192) == _schedule(lv, 12, 0, 1, 8192)     # 4 IS a boundary of that schedule: nothing changes
    assert build_then_add_schedule(1, 1, 2)(lv, 4, 7, 1, 8192) == [(1, 2, 0, 1, False), (2, 4, 0, 1, False)]
