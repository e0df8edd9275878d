"""GPU: HNSW graph construction (cvtmi_hnsw_build, csrc/hnsw_build.hip) and saveIndex (cvtmi_hnsw_save).

max_batch = 1 is the reference's sequential insertion: the saved file is compared byte for byte with the golden graphs the reference
wrote, with the reference compiled in place (oracle/_ref, where built), and with the host mirror's sequential build (the hnsw_build
CLI, itself pinned to the reference by tests/test_host_hnsw_build.py).  Larger batches give a different, deterministic graph.  What
that graph must be, byte for byte, is checked in tests/test_gpu_hnsw_build_batches.py against a Python model of DESIGN 4.11
(tests/hnsw_build_model.py, pinned on the CPU by tests/test_hnsw_build_model.py) on graphs of a few thousand rows; the graphs here
are beyond that model's reach and are checked for determinism, soundness, agreement of the GPU search with the reference's
searchKnn on the saved file, and recall."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
CASES = ("ip32", "l2f16", "ip20", "l2f7", "ip128")
HAVE_REF = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libref_hnsw.so"))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available()
    import cvt_amd
    return cvt_amd


def parse(blob):
    """header fields, rows, labels, per-element level count, level-0 lists, upper lists {(node, level): list}"""
    blob = np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else blob
    off0, cap, cnt, per, offl, offd = struct.unpack("<6Q", blob[:48].tobytes())
    maxlevel, ep = struct.unpack("<iI", blob[48:56].tobytes())
    maxM, maxM0, M = struct.unpack("<3Q", blob[56:80].tobytes())
    D = (offl - offd) // 4
    body = blob[96:96 + cap * per].reshape(cap, per)[:cnt]
    l0 = body[:, :4 + 4 * maxM0].copy().view(np.uint32)
    rows = body[:, offd:offl].copy().view(np.float32)
    labels = body[:, offl:offl + 8].copy().view(np.uint64).ravel()
    p = 96 + cap * per
    levels, sizes, upper = [], [], {}
    for i in range(cap):
        sz = int(blob[p:p + 4].view(np.uint32)[0]); p += 4
        sizes.append(sz)
        nl = sz // (4 * maxM + 4)
        if i < cnt:
            levels.append(nl)
            words = blob[p:p + sz].view(np.uint32).reshape(nl, maxM + 1) if nl else None
            for lv in range(1, nl + 1):
                upper[(i, lv)] = words[lv - 1]
        p += sz
    assert p == blob.size
    return dict(cnt=int(cnt), cap=int(cap), maxlevel=maxlevel, ep=ep, maxM=int(maxM), maxM0=int(maxM0), M=int(M), D=int(D),
                rows=rows, labels=labels, levels=np.array(levels), sizes=sizes, l0=l0, upper=upper)


def assert_sound(g):
    n = g["cnt"]
    lv = g["levels"]
    deg = g["l0"][:, 0]
    assert deg.max() <= g["maxM0"]
    if n > 1:
        assert deg.min() >= 1
    for i in range(n):
        nb = g["l0"][i, 1:1 + deg[i]]
        assert (nb < n).all() and i not in nb and len(set(nb.tolist())) == len(nb), i
    for (i, l), u in g["upper"].items():
        c = int(u[0])
        assert c <= g["maxM"]
        nb = u[1:1 + c]
        assert (nb < n).all() and i not in nb and len(set(nb.tolist())) == len(nb), (i, l)
        assert (lv[nb] >= l).all(), (i, l)
    assert g["maxlevel"] == lv.max() and lv[g["ep"]] == g["maxlevel"]


def gpu_build(amd, x, metric, M, efc, labels=None, max_batch=1):
    return np.frombuffer(amd.hnsw_build(x, metric, M, efc, labels=labels, max_batch=max_batch).save(), dtype=np.uint8)


def host_build(tmp_path, x, metric, M, efc, name, threads=None):
    """the host mirror's build: sequential (threads None: one addPoint per row), or addPoints with `threads` workers"""
    rf = tmp_path / (name + "_rows.bin"); rf.write_bytes(np.ascontiguousarray(x, np.float32).tobytes())
    out = tmp_path / (name + ".hnsw")
    cmd = [os.path.join(BIN, "hnsw_build"), str(rf), str(x.shape[1]), str(M), str(efc), str(out), "l2" if metric == 1 else "ip"]
    if threads is not None:
        cmd += ["-", str(threads)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(out, dtype=np.uint8)


def tie_heavy(n, D, seed):
    rng = np.random.default_rng(seed)
    x = np.round(rng.normal(size=(n, D)) * 4).astype(np.float32) / 4
    x[n // 2:n // 2 + 200] = x[:200]
    return x


# ---- 1. golden graphs, sequential ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_sequential_build_rebuilds_golden_graph(amd, golden, case):
    g = golden.hnsw
    blob = g[case + "_index"]
    metric, D, n, M, efc, k, ef = (int(v) for v in g[case + "_meta"])
    p = parse(blob)
    out = gpu_build(amd, p["rows"], metric, M, efc, labels=p["labels"], max_batch=1)
    assert out.size == blob.size and np.array_equal(out, blob)


# ---- 2. the reference's fresh sequential build, tie-heavy rows ---------------------------------------------------------------------
@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref not built (needs the reference tree at build time)")
@pytest.mark.parametrize("metric,D,n,M,efc", [(0, 64, 5000, 16, 100), (1, 32, 5000, 5, 40), (1, 10, 4000, 24, 30), (0, 20, 3000, 24, 50)])
def test_sequential_build_matches_reference(amd, tmp_path, metric, D, n, M, efc):
    from oracle import binding as ob
    x = tie_heavy(n, D, 1000 + D)
    path = str(tmp_path / "ref.hnsw")
    ob.RefHnsw().build(metric, x, path, M, efc, threads=1)
    ref = np.fromfile(path, dtype=np.uint8)
    out = gpu_build(amd, x, metric, M, efc, max_batch=1)
    assert out.size == ref.size and np.array_equal(out, ref)


# ---- 3. load -> save ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_load_save_round_trip(amd, golden, case):
    g = golden.hnsw
    blob = g[case + "_index"]
    metric, D = int(g[case + "_meta"][0]), int(g[case + "_meta"][1])
    idx = amd.HnswIndex(blob.tobytes(), metric, D)
    assert np.array_equal(np.frombuffer(idx.save(), dtype=np.uint8), blob)


def test_save_of_spare_capacity_writes_zeros(amd, golden):
    """a file with max_elements > cur_element_count: the spare slots come back as zeros, the rest unchanged"""
    if not HAVE_REF:
        pytest.skip("oracle/_ref not built")
    import tempfile
    from oracle import binding as ob
    p = parse(golden.hnsw["l2f7_index"])
    src = p["rows"]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "spare.hnsw")
        ob.RefHnsw().build(1, src, path, 4, 20, labels=p["labels"].view(np.int64), max_elements=p["cnt"] + 10)
        spare = np.fromfile(path, dtype=np.uint8)
    out = np.frombuffer(amd.HnswIndex(spare.tobytes(), 1, 7).save(), dtype=np.uint8)
    assert out.size == spare.size
    q = parse(out)
    assert q["cap"] == p["cnt"] + 10 and q["cnt"] == p["cnt"]
    per = 4 + 4 * q["maxM0"] + 4 * 7 + 8
    body = out[96:96 + q["cap"] * per].reshape(q["cap"], per)
    assert not body[q["cnt"]:].any() and q["sizes"][q["cnt"]:] == [0] * 10
    assert np.array_equal(body[:q["cnt"]], spare[96:96 + q["cap"] * per].reshape(q["cap"], per)[:q["cnt"]])
    assert np.array_equal(out[:96], spare[:96])


# ---- 4. default schedule -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows50k():
    rng = np.random.default_rng(44)
    cen = rng.normal(size=(200, 32)).astype(np.float32)
    x = cen[rng.integers(0, 200, 50000)] + 0.5 * rng.normal(size=(50000, 32)).astype(np.float32)
    q = x[rng.integers(0, 50000, 300)] + 0.1 * rng.normal(size=(300, 32)).astype(np.float32)
    return x.astype(np.float32), q.astype(np.float32)


@pytest.mark.parametrize("metric", [0, 1])
def test_default_schedule(amd, tmp_path, rows50k, metric):
    import torch
    x, q = rows50k
    M, efc = 12, 64
    labels = (np.arange(x.shape[0], dtype=np.uint64) * 7 + 3)
    a = gpu_build(amd, x, metric, M, efc, labels=labels, max_batch=0)
    b = gpu_build(amd, x, metric, M, efc, labels=labels, max_batch=0)
    assert np.array_equal(a, b)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xd = torch.from_numpy(x).cuda()
        ld = torch.from_numpy(labels.view(np.int64)).cuda()
        idx = amd.hnsw_build(xd, metric, M, efc, labels=ld, max_batch=0)
    s.synchronize()
    c = np.frombuffer(idx.save(), dtype=np.uint8)
    assert np.array_equal(a, c)
    # rows, labels and level sizes are those of the sequential file (same ids, same level draws)
    seq = parse(host_build(tmp_path, x, metric, M, efc, "seq", threads=8))
    g = parse(a)
    assert np.array_equal(g["rows"].view(np.uint32), x.view(np.uint32)) and np.array_equal(g["labels"], labels)
    assert g["sizes"] == seq["sizes"] and g["maxlevel"] == seq["maxlevel"] and g["ep"] == seq["ep"]
    assert a[:96].tobytes() == seq_header(tmp_path, x, metric, M, efc)
    assert_sound(g)
    # search on the built handle = the reference's searchKnn on the saved file
    d, lab = idx.search(q, 10, 64)
    if HAVE_REF:
        from oracle import binding as ob
        path = str(tmp_path / "built.hnsw")
        a.tofile(path)
        rd, rl = ob.RefHnsw().search(metric, x.shape[1], path, q, 10, 64)
        assert np.array_equal(rl, lab) and np.array_equal(rd.view(np.uint32), d.view(np.uint32))
    d2, lab2 = amd.HnswIndex(a.tobytes(), metric, x.shape[1]).search(q, 10, 64)
    assert np.array_equal(lab2, lab) and np.array_equal(d2.view(np.uint32), d.view(np.uint32))


_headers = {}


def seq_header(tmp_path, x, metric, M, efc):
    """the first 96 bytes of a host build of the same rows (header: counts, sizes, top level, entry, M, mult, ef_construction)"""
    key = (x.shape, metric, M, efc)
    if key not in _headers:
        _headers[key] = host_build(tmp_path, x, metric, M, efc, "hdr", threads=8)[:96].tobytes()
    return _headers[key]


# ---- 5. quality ------------------------------------------------------------------------------------------------------------------
def config5_rows(n, D=128, nq=1000):
    rng = np.random.default_rng(5)
    cen = rng.normal(size=(1000, D)).astype(np.float32)
    x = cen[rng.integers(0, 1000, n)] + 0.6 * rng.normal(size=(n, D)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = x[rng.integers(0, n, nq)] + 0.15 * rng.normal(size=(nq, D)).astype(np.float32)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(x, np.float32), q


def recall(amd, blob, metric, D, q, truth, ef):
    _, lab = amd.HnswIndex(blob.tobytes(), metric, D).search(q, 10, ef)
    r1 = float((lab[:, 0] == truth[:, 0]).mean())
    r10 = float(np.mean([len(set(lab[i]) & set(truth[i])) / 10.0 for i in range(len(q))]))
    return r1, r10


@pytest.mark.parametrize("metric", [0, 1])
def test_recall_matches_host_build(amd, tmp_path, metric):
    """The host graph is the sequential one (one addPoint per row: the reference's own file, a fixed graph).  A 16-thread host build
    depends on how its threads interleave, and on these rows its recall@10 at ef = 64 moved between 0.723 and 0.753 over six
    builds, three times the 0.01 allowed here, around the sequential graph's 0.7397; the GPU graph is a fixed 0.7355."""
    import torch
    x, q = config5_rows(100_000)
    xd, qd = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
    if metric == 0:
        truth = torch.topk(qd @ xd.T, 10, dim=1).indices.cpu().numpy()
    else:
        truth = torch.topk(-torch.cdist(qd, xd), 10, dim=1).indices.cpu().numpy()
    gpu = gpu_build(amd, x, metric, 16, 40, max_batch=0)
    host = host_build(tmp_path, x, metric, 16, 40, "host")
    rg = recall(amd, gpu, metric, 128, q, truth, 64)
    rh = recall(amd, host, metric, 128, q, truth, 64)
    assert rg[0] >= rh[0] - 0.01 and rg[1] >= rh[1] - 0.01, (rg, rh)


# ---- 6. edge cases (max_batch = 1 against the host mirror's sequential file, default schedule sound) --------------------------------
@pytest.mark.parametrize("shape", ["n1", "n2", "n_lt_M", "identical", "d7", "raise"])
def test_edge_cases(amd, tmp_path, shape):
    rng = np.random.default_rng(77)
    M, efc, metric = 8, 20, 1
    if shape == "n1":
        x = rng.normal(size=(1, 16))
    elif shape == "n2":
        x = rng.normal(size=(2, 16))
    elif shape == "n_lt_M":
        x = rng.normal(size=(5, 16))
    elif shape == "identical":
        x = np.repeat(rng.normal(size=(1, 16)), 300, axis=0); metric = 0
    elif shape == "d7":
        x = rng.normal(size=(900, 7))
    else:
        x = rng.normal(size=(3000, 24)); M, efc = 4, 16
    x = np.ascontiguousarray(x, np.float32)
    seq = host_build(tmp_path, x, metric, M, efc, shape)
    out = gpu_build(amd, x, metric, M, efc, max_batch=1)
    assert np.array_equal(out, seq)
    g = parse(out)
    if shape == "raise":   # some row after the first raises the top level (and so ends its batch in the default schedule)
        lv = g["levels"]
        assert any(lv[i] > lv[:i].max() for i in range(1, len(lv)))
    dflt = parse(gpu_build(amd, x, metric, M, efc, max_batch=0))
    assert dflt["sizes"] == g["sizes"] and dflt["ep"] == g["ep"]
    assert_sound(dflt)


# ---- 7. other batch caps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_batch", [2, 7, 64])
def test_batch_caps_give_sound_graphs(amd, rows50k, max_batch):
    x, q = rows50k
    x = x[:20000]
    a = gpu_build(amd, x, 1, 10, 40, max_batch=max_batch)
    assert np.array_equal(a, gpu_build(amd, x, 1, 10, 40, max_batch=max_batch))
    g = parse(a)
    assert_sound(g)
    _, lab = amd.HnswIndex(a.tobytes(), 1, 32).search(q, 1, 64)
    exact = ((q[:, None, :] - x[None, :, :]) ** 2).sum(-1).argmin(1)
    assert float((lab[:, 0] == exact).mean()) > 0.9


# ---- the hnsw_build CLI (host mirror: HierarchicalNSW::addPointsGpu + cvtmi_hnsw_save) -----------------------------------------------
@pytest.mark.parametrize("mode", ["gpu:1", "gpu"])
def test_cli_gpu_mode(amd, tmp_path, golden, mode):
    g = golden.hnsw
    blob = g["l2f16_index"]
    metric, D, n, M, efc, k, ef = (int(v) for v in g["l2f16_meta"])
    p = parse(blob)
    rf = tmp_path / "rows.bin"; rf.write_bytes(p["rows"].tobytes())
    lf = tmp_path / "labels.bin"; lf.write_bytes(p["labels"].tobytes())
    out = tmp_path / "out.hnsw"
    r = subprocess.run([os.path.join(BIN, "hnsw_build"), str(rf), str(D), str(M), str(efc), str(out), "l2", str(lf), mode],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(out, dtype=np.uint8)
    expect = blob if mode == "gpu:1" else gpu_build(amd, p["rows"], metric, M, efc, labels=p["labels"], max_batch=0)
    assert np.array_equal(got, expect)
