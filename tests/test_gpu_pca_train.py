"""GPU: PCA training (cvtmi_pca_covariance / cvtmi_pca_train; cv::PCA(data, noArray(), DATA_AS_ROW, dout) in the
reference's train/src/train.cpp).  OpenCV is absent here: PARITY UNPINNED.  The library states its own arithmetic
(include/cvtmi.h, "PCA training") and is held to it against float64 numpy with rigorous bounds.  `d` is always the
rows centred in numpy float32 with the mean the library returned."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
U52, U53, U24 = 2.0 ** -52, 2.0 ** -53, 2.0 ** -24


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()  # raises if the HIP library is missing: there is no fallback
    return cvt_amd


def cnn_like(rng, n, d):
    x = np.maximum(rng.normal(size=(n, d)), 0).astype(np.float32) * rng.gamma(2.0, 1.0, size=(1, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def ulp_diff(a, b):
    ia = a.view(np.int32).astype(np.int64); ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia); ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def check_covariance(x, mean, cov):
    n, din = x.shape
    want_mean = x.astype(np.float64).mean(axis=0).astype(np.float32)
    assert ulp_diff(mean, want_mean).max() <= 1
    assert cov.dtype == np.float64 and cov.shape == (din, din)
    assert np.array_equal(cov.view(np.uint64), cov.T.view(np.uint64)), "cov is not bitwise symmetric"
    d = (x - mean[None, :]).astype(np.float32).astype(np.float64)
    want = d.T @ d / n
    bound = (n + 1) * U52 * (np.abs(d).T @ np.abs(d)) / n
    err = np.abs(cov - want)
    assert np.all(err <= bound), "worst excess %g" % (err - bound).max()


@pytest.mark.parametrize("n,din", [(1, 4), (7, 4), (1000, 20), (4097, 128), (65537, 64), (30000, 1024), (20000, 2048)])
def test_covariance_contract(amd, n, din):
    import torch
    rng = np.random.default_rng(n * 7 + din)
    x = (rng.normal(size=(n, din)) * rng.uniform(0.1, 3.0, size=din) + rng.normal(size=din)).astype(np.float32)
    mean, cov = amd.pca_covariance(x)
    check_covariance(x, mean, cov)
    mean2, cov2 = amd.pca_covariance(x)
    assert np.array_equal(mean.view(np.uint32), mean2.view(np.uint32)) and np.array_equal(cov.view(np.uint64), cov2.view(np.uint64))
    dm, dc = amd.pca_covariance(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(mean.view(np.uint32), dm.cpu().numpy().view(np.uint32))
    assert np.array_equal(cov.view(np.uint64), dc.cpu().numpy().view(np.uint64))


def test_large_offset_small_spread(amd):
    """x = 1000 + 0.1 z: the uncentred one-pass form X^T X / n - mu mu^T loses ~(1000 / 0.1)^2 of its accuracy here"""
    rng = np.random.default_rng(0x0FF5E7)
    x = (1000.0 + 0.1 * rng.normal(size=(50000, 64))).astype(np.float32)
    mean, cov = amd.pca_covariance(x)
    check_covariance(x, mean, cov)
    assert np.abs(np.diag(cov) - 0.01).max() < 1e-3


def spectrum_rows(rng, n, din):
    q = np.linalg.qr(rng.normal(size=(din, din)))[0]
    sigma = np.geomspace(1.0, 0.01, din)
    mu = rng.normal(size=din)
    return (mu + (rng.normal(size=(n, din)) * sigma) @ q.T).astype(np.float32)


def check_model(cov, vectors, values, dout):
    din = cov.shape[0]
    lam_all, V = np.linalg.eigh(cov)
    full = lam_all[::-1]
    lam, V = full[:dout], V[:, ::-1][:, :dout].T
    norm = np.abs(lam_all).max()
    assert vectors.shape == (dout, din) and values.shape == (dout,)
    assert np.all(np.diff(values) <= 0), "values not descending"
    assert np.all(np.abs(values.astype(np.float64) - lam) <= U24 * np.abs(lam) + 64 * din * U53 * norm)
    v = vectors.astype(np.float64)
    # sign: the largest-magnitude component is positive (its float image, so ties after rounding cannot mislead)
    assert np.all(v.max(axis=1) == np.abs(v).max(axis=1))
    gap = np.array([np.min(np.abs(np.delete(full, k) - full[k])) for k in range(dout)])
    V = V * np.sign(np.sum(V * v, axis=1))[:, None]
    ok = gap >= 1e-3 * norm
    assert ok.sum() >= 1
    err = np.abs(v - V).max(axis=1)
    assert np.all(err[ok] <= 1e-6 + 64 * din * U53 * norm / gap[ok]), "worst %g" % err[ok].max()
    assert np.abs(v @ v.T - np.eye(dout)).max() <= 4 * din * U24


@pytest.mark.parametrize("din,dout", [(128, 128), (128, 16), (1024, 256), (2048, 256)])
def test_spectrum(amd, din, dout):
    rng = np.random.default_rng(din + dout)
    x = spectrum_rows(rng, 2 * din + 3, din)
    mean, cov = amd.pca_covariance(x)
    m2, vectors, values = amd.pca_train(x, dout)
    assert np.array_equal(mean.view(np.uint32), m2.view(np.uint32))
    check_model(cov, vectors, values, dout)


def test_device_entry(amd):
    import torch
    rng = np.random.default_rng(5)
    x = spectrum_rows(rng, 3000, 256)
    m, v, l = amd.pca_train(x, 64)
    dm, dv, dl = amd.pca_train(torch.from_numpy(x).cuda(), 64)
    torch.cuda.synchronize()
    assert np.array_equal(m.view(np.uint32), dm.cpu().numpy().view(np.uint32))
    _, cov = amd.pca_covariance(x)
    check_model(cov, dv.cpu().numpy(), dl.cpu().numpy(), 64)
    assert np.abs(dv.cpu().numpy() - v).max() < 1e-5 and np.abs(dl.cpu().numpy() - l).max() <= 1e-6 * l[0]


def test_train_then_project(amd):
    rng = np.random.default_rng(0x7A1)
    x = cnn_like(rng, 20000, 1024)
    mean, vectors, values = amd.pca_train(x, 128)
    y = amd.pca_project(mean, vectors, x, l2norm=False).astype(np.float64)
    y -= y.mean(axis=0)
    cy = y.T @ y / len(x)
    assert np.abs(cy - np.diag(values.astype(np.float64))).max() <= 1e-5 * values[0]


def read_yaml_matrix(text, name):
    m = re.search(r"^%s: !!opencv-matrix\n   rows: (\d+)\n   cols: (\d+)\n   dt: f\n   data: \[([^\]]*)\]" % name, text, re.M)
    assert m, name
    vals = np.array([float(t) for t in m.group(3).replace(",", " ").split()], dtype=np.float64).astype(np.float32)
    return vals.reshape(int(m.group(1)), int(m.group(2)))


def test_host_mirror_and_cli(amd, tmp_path):
    exe = os.path.join(BIN, "pca_train")
    assert os.path.exists(exe), "host CLIs not built: __graft_entry__.build()"
    rng = np.random.default_rng(0xC11)
    din, dout = 64, 16
    x = cnn_like(rng, 500, din)
    with open(tmp_path / "feats.txt", "w") as f:
        for i, row in enumerate(x):
            f.write("f%d," % i + ",".join("%.9g" % v for v in row) + "\n")
            if i == 10:
                f.write("short," + ",".join("%.9g" % v for v in row[:din - 1]) + "\n")
    model = tmp_path / "model.yml"
    r = subprocess.run([exe, str(tmp_path / "feats.txt"), str(model), str(din), str(dout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "1 lines skipped: feat size != 64" in r.stdout and "500 rows trained 64 -> 16" in r.stdout
    text = model.read_text()
    assert text.startswith("%YAML:1.0\n---\nname: PCA\nvectors: !!opencv-matrix\n")
    vec, val, mu = (read_yaml_matrix(text, k) for k in ("vectors", "values", "mean"))
    assert vec.shape == (dout, din) and val.shape == (dout, 1) and mu.shape == (1, din)
    # 9 significant digits: the text is exactly the image of the floats it was written from
    for name, m in (("vectors", vec), ("values", val), ("mean", mu)):
        body = re.search(r"^%s: .*?data: \[([^\]]*)\]" % name, text, re.M | re.S).group(1)
        assert body.replace(",", " ").split() == ["%.8e" % v for v in m.ravel()]
    # PCAUtils::loadModel reads the same floats
    r = subprocess.run([os.path.join(BIN, "pca_project"), str(model), "--info"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    sv = np.cumsum(vec.astype(np.float64).ravel())[-1]; sm = np.cumsum(mu.astype(np.float64).ravel())[-1]
    assert r.stdout.strip() == "vectors %d x %d sum %.9g; values %d x 1; mean 1 x %d sum %.9g" % (dout, din, sv, dout, din, sm)
    # the same model as the Python binding: the mean and covariance bit for bit; the eigensolver may be another build of
    # rocSOLVER in this process (the one PyTorch ships) than in the tool's, so the eigenpairs are held to the solver bounds
    mean, vectors, values = amd.pca_train(x, dout)
    assert np.array_equal(mu[0].view(np.uint32), mean.view(np.uint32))
    _, cov = amd.pca_covariance(x)
    check_model(cov, vec, val[:, 0], dout)
    assert np.abs(vec - vectors).max() < 1e-5 and np.abs(val[:, 0] - values).max() <= 1e-6 * values[0]
    # and the written model projects end to end
    r = subprocess.run([os.path.join(BIN, "pca_project"), str(model), str(tmp_path / "feats.txt"), str(tmp_path / "out.txt")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "holds 63 values" in r.stdout  # pca_project takes no short rows
    with open(tmp_path / "good.txt", "w") as f:
        for i, row in enumerate(x[:50]):
            f.write("f%d," % i + ",".join("%.9g" % v for v in row) + "\n")
    r = subprocess.run([os.path.join(BIN, "pca_project"), str(model), str(tmp_path / "good.txt"), str(tmp_path / "out.txt")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    y = np.array([[float(t) for t in line.split()[1:]] for line in open(tmp_path / "out.txt")])
    want = amd.pca_project(mu[0], vec, x[:50], l2norm=True)
    assert y.shape == (50, dout) and np.abs(y - want).max() < 1e-8


def test_errors(amd):
    lib = amd.lib()
    x = np.ones((8, 16), np.float32)
    mean = np.empty(16, np.float32); cov = np.empty((16, 16)); vec = np.empty((16, 16), np.float32); val = np.empty(16, np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    null = C.c_void_p(0)
    cases = [
        ("covariance", (p(x), C.c_int64(8), C.c_int(14), p(mean), p(cov)), "multiple of 4"),
        ("covariance", (p(x), C.c_int64(2), C.c_int(2052), p(mean), p(cov)), "multiple of 4"),
        ("covariance", (p(x), C.c_int64(0), C.c_int(16), p(mean), p(cov)), "n = 0"),
        ("covariance", (null, C.c_int64(8), C.c_int(16), p(mean), p(cov)), "null pointer"),
        ("covariance", (p(x), C.c_int64(8), C.c_int(16), p(mean), null), "null pointer"),
        ("train", (p(x), C.c_int64(8), C.c_int(16), C.c_int(17), p(mean), p(vec), p(val)), "dout = 17"),
        ("train", (p(x), C.c_int64(8), C.c_int(16), C.c_int(9), p(mean), p(vec), p(val)), "dout = 9"),
        ("train", (p(x), C.c_int64(8), C.c_int(16), C.c_int(0), p(mean), p(vec), p(val)), "dout = 0"),
        ("train", (p(x), C.c_int64(0), C.c_int(16), C.c_int(1), p(mean), p(vec), p(val)), "n = 0"),
        ("train", (p(x), C.c_int64(8), C.c_int(2048 + 4), C.c_int(1), p(mean), p(vec), p(val)), "multiple of 4"),
        ("train", (p(x), C.c_int64(8), C.c_int(16), C.c_int(4), p(mean), p(vec), null), "null pointer"),
        ("train", (null, C.c_int64(8), C.c_int(16), C.c_int(4), p(mean), p(vec), p(val)), "null pointer"),
    ]
    for kind, args, msg in cases:
        for dev in (False, True):
            fn = getattr(lib, "cvtmi_pca_%s%s" % (kind, "_dev" if dev else ""))
            rc = fn(*args, null) if dev else fn(*args)
            assert rc == -1, (kind, dev, msg, rc)
            assert msg in lib.cvtmi_last_error().decode(), (kind, dev, lib.cvtmi_last_error())
    # a good call still works after the failures
    m, v, vals = amd.pca_train(cnn_like(np.random.default_rng(1), 64, 16), 4)
    assert v.shape == (4, 16) and np.all(np.diff(vals) <= 0)
