"""GPU: cvtmi_hnsw_build with batches of more than one row, byte for byte against tests/hnsw_build_model.py.

The model restates DESIGN 4.11 in Python and is pinned on the CPU (tests/test_hnsw_build_model.py): at max_batch = 1 to the golden
graphs the reference wrote and to the host mirror, and each shape of the shared table to the batch-only path it is there for --
several proposals per (target, level), repeated re-selection of one full list, appends into slots a re-selection freed, targets
with proposals on several levels, 65-candidate re-selections, more than 2048 proposals for one target, batches cut by a row that
raises the top level, result queues shorter than M, ties throughout.  Levels and header come from the host mirror's sequential
build of the same rows, never from the build under test.  The whole file is compared: no tolerance, no node left out."""
import time

import numpy as np
import pytest

import hnsw_build_model as hm
from test_gpu_hnsw_build import host_build, parse

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available()
    import cvt_amd
    return cvt_amd


_models = {}


def model_of(orc, tmp_path, name):
    if name not in _models:
        c = hm.CASES[name]
        x = c["rows"]()
        labels = c["labels"](x.shape[0]) if "labels" in c else None
        seq = host_build(tmp_path, x, c["metric"], c["M"], c["efc"], "seq_" + name)
        want, cnt = hm.build_model(orc, x, c["metric"], c["M"], c["efc"], parse(seq)["levels"], labels, c["max_batch"],
                                   c.get("frac", 32), vectorised=True)
        assert want[:96] == seq[:96].tobytes()
        _models[name] = (x, labels, np.frombuffer(want, dtype=np.uint8), cnt)
    return _models[name]


def explain(got, want, cnt):
    if got.size != want.size:
        return "file sizes differ: %d, model %d" % (got.size, want.size)
    diff = hm.first_difference(parse(got), parse(want), cnt)
    if diff is None:
        return "link lists agree; first differing byte %d" % int(np.flatnonzero(got != want)[0])
    return "first difference at (node, level) %s: built %s, model %s, last touched by the model's batch %s" % diff


@pytest.mark.parametrize("name", list(hm.CASES))
def test_batched_build_is_the_model(amd, orc, tmp_path, name):
    import torch
    c = hm.CASES[name]
    x, labels, want, cnt = model_of(orc, tmp_path, name)
    assert c["need"](cnt)
    try:
        amd.set_tuning("hnsw_build_frac", c.get("frac", 32))
        amd.set_tuning("hnsw_build_cap", 8192)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx = amd.hnsw_build(x, c["metric"], c["M"], c["efc"], labels=labels, max_batch=c["max_batch"])
        ms = (time.perf_counter() - t0) * 1e3
        got = np.frombuffer(idx.save(), dtype=np.uint8)
        print("%s: %d rows, %d batches (largest %d), GPU build %.1f ms" % (name, x.shape[0], cnt["batches"], cnt["largest_batch"], ms))
        assert np.array_equal(got, want), explain(got, want, cnt)
        if c.get("device"):   # the device-pointer entry, rows and labels on the device, on a side stream
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                xd = torch.from_numpy(x).cuda()
                ld = torch.from_numpy(labels.view(np.int64)).cuda()
                idx = amd.hnsw_build(xd, c["metric"], c["M"], c["efc"], labels=ld, max_batch=c["max_batch"])
            s.synchronize()
            got = np.frombuffer(idx.save(), dtype=np.uint8)
            assert np.array_equal(got, want), explain(got, want, cnt)
    finally:
        amd.set_tuning("hnsw_build_frac", 32)
        amd.set_tuning("hnsw_build_cap", 8192)
