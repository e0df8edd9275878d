"""CPU: deletion in the host mirror (cvt_amd/host/hnswlib/hnswalg.h: markDelete / unmarkDelete, the mark in parse / saveIndex, addPoint
on a graph with marked nodes) through the hnsw_delete and hnsw_add CLIs, on the golden graphs.

  * hnsw_delete changes bit 16 of the marked nodes' level-0 count words and nothing else; --unmark restores the file; a marked file
    passes through loadIndex / saveIndex unchanged (hnsw_delete with an empty label set is exactly that round trip).
  * hnsw_delete + hnsw_add (host: one addPoint per row) writes, byte for byte, the file of the Python model of DESIGN 4.7.2
    (tests/hnsw_delete_model.py) at batch size 1, for the dead sets: the entry point alone, a random third, every node but one, every
    node, and no node -- which is the file hnsw_add writes today.

No device is needed: hnsw_delete and hnsw_add in host mode never upload the graph.  The helpers are shared with
tests/test_gpu_hnsw_delete.py."""
import os
import subprocess

import numpy as np
import pytest

import hnsw_delete_model as dm
from test_gpu_hnsw_build import CASES as GOLDEN, parse
from test_host_hnsw_add import host_add

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
DEAD_SETS = ("entry", "third", "all_but_one", "all", "none")


def host_delete(tmp_path, index, labels, name, unmark=False):
    """hnsw_delete: the bytes of the file it writes, and the line it prints"""
    exe = os.path.join(BIN, "hnsw_delete")
    assert os.path.exists(exe), "host CLIs not built: __graft_entry__.build()"
    src = tmp_path / (name + "_del_in.hnsw"); src.write_bytes(bytes(index))
    lf = tmp_path / (name + "_del_labels.txt"); lf.write_text("".join("%d\n" % int(v) for v in labels))
    out = tmp_path / (name + "_del_out.hnsw")
    r = subprocess.run([exe, str(src), str(lf), str(out)] + (["--unmark"] if unmark else []), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(out, dtype=np.uint8), r.stdout


def dead_set(name, p, seed=5):
    """the nodes of a parsed graph that a named dead set deletes, ascending"""
    n = p["cnt"]
    if name == "entry":
        return np.array([p["ep"]], dtype=np.int64)
    if name == "third":
        return np.sort(np.random.default_rng(seed).choice(n, n // 3, replace=False))
    if name == "all_but_one":
        return np.delete(np.arange(n), n // 2)
    if name == "all":
        return np.arange(n)
    return np.zeros(0, dtype=np.int64)


def extra_rows(p, m, seed):
    """m new rows near the graph's own (some of them copies: distance 0 to a node that may be dead)"""
    rng = np.random.default_rng(seed)
    x = p["rows"][rng.integers(0, p["cnt"], m)] + (rng.normal(size=(m, p["D"])) * 0.25).astype(np.float32)
    x[::7] = p["rows"][rng.integers(0, p["cnt"], len(x[::7]))]
    return np.ascontiguousarray(x, np.float32)


def count_words(blob):
    p = parse(blob)
    return p["l0"][:, 0].copy()


@pytest.mark.parametrize("case", GOLDEN)
def test_marks_are_bit_16_and_round_trip(tmp_path, golden, case):
    blob = golden.hnsw[case + "_index"]
    p = parse(blob)
    n = p["cnt"]
    dead = dead_set("third", p)
    labels = np.concatenate([p["labels"][dead], p["labels"][dead[:5]], np.array([2 ** 63 + 12345], np.uint64)])   # duplicates, a foreign label
    marked, said = host_delete(tmp_path, blob, labels, case)
    assert "%d nodes marked, %d of %d deleted" % (len(dead), len(dead), n) in said
    assert np.array_equal(marked, dm.with_marks(blob, dead))
    diff = count_words(marked) ^ count_words(blob)
    assert np.array_equal(np.flatnonzero(diff), dead) and (diff[dead] == dm.DELETE_BIT).all()
    assert np.array_equal(dm.dead_of(marked), dead)
    # loadIndex / saveIndex alone, marking again, unmarking
    again, said = host_delete(tmp_path, marked, [], case + "_rt")
    assert np.array_equal(again, marked) and "0 nodes marked, %d of %d deleted" % (len(dead), n) in said
    again, said = host_delete(tmp_path, marked, labels, case + "_twice")
    assert np.array_equal(again, marked) and "0 nodes marked" in said
    half = dead[::2]
    some, said = host_delete(tmp_path, marked, p["labels"][half], case + "_half", unmark=True)
    assert "%d nodes unmarked" % len(half) in said and np.array_equal(some, dm.with_marks(blob, np.setdiff1d(dead, half)))
    back, _ = host_delete(tmp_path, marked, labels, case + "_back", unmark=True)
    assert np.array_equal(back, blob)


def test_corrupt_mark_bits_are_refused(tmp_path, golden):
    blob = golden.hnsw["l2f7_index"].copy()
    per = parse(blob)["l0"].shape[1] * 4 + parse(blob)["D"] * 4 + 8
    blob[96 + 3 * per + 2] |= 2      # bit 17 of node 3's count word
    src = tmp_path / "bad.hnsw"; src.write_bytes(blob.tobytes())
    lf = tmp_path / "none.txt"; lf.write_text("")
    r = subprocess.run([os.path.join(BIN, "hnsw_delete"), str(src), str(lf), str(tmp_path / "out.hnsw")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "corrupt link count" in r.stdout


@pytest.mark.parametrize("which", DEAD_SETS)
@pytest.mark.parametrize("case", GOLDEN)
def test_host_add_on_a_marked_graph_is_the_model(orc, tmp_path, golden, case, which):
    g = golden.hnsw
    blob = g[case + "_index"]
    metric, D, n, M, efc, k, ef = (int(v) for v in g[case + "_meta"])
    p = parse(blob)
    dead = dead_set(which, p)
    extra = extra_rows(p, 24, 100 + D)
    labels = np.arange(24, dtype=np.uint64) + 10 ** 7
    marked, _ = host_delete(tmp_path, blob, p["labels"][dead], case + which)
    got = host_add(tmp_path, marked, extra, D, metric, case + which, labels=labels)
    levels = parse(got)["levels"][n:]
    want, cnt = dm.add_model(orc, marked, metric, extra, levels, labels, 1)
    print("%s / %s: %d dead of %d, model counters %s" % (case, which, len(dead), n, cnt))
    assert got.size == want.size and np.array_equal(got, want)
    assert np.array_equal(dm.dead_of(got), dead)                     # marks kept, new rows live
    if which == "none":     # today's bytes: the unmarked file through hnsw_add
        assert np.array_equal(marked, blob) and cnt["past_stop"] == 0 and cnt["ep_pushes"] == 0
    else:
        assert cnt["ep_pushes"] > 0 or which == "third"
        new_links = parse(got)["l0"][n:]
        for row in new_links:          # a new row links to live nodes only, but for the dead entry point offered after the walk
            nb = row[1:1 + (row[0] & 0xffff)]
            assert np.isin(nb, dead).sum() <= (1 if p["ep"] in dead else 0)
