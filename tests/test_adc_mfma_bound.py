"""The error bound of the int8 matrix-core ADC filter (adc_mfma.hip, restated in adc_mfma_model.py), against the oracle's own fp32
arithmetic: for every (row, query), |d_ref - (C_q - 2 t a)| <= E_q, where d_ref is the oracle's table + scan sum (orc.lut, orc.adc_scan:
what adc_search ranks) and a the exact integer the filter kernels compute.  The filter is only safe while this holds, whatever the
codebooks and the batch look like -- the cases are the ones where the quantisation is at its worst."""
import numpy as np
import pytest

from adc_mfma_model import Batch, IndexModel

M, ROWS, NQ = 16, 300, 12


def _books(rng, K, step, scale=1.0, offset=0.0):
    return (rng.standard_normal((M, K, step)) * scale + offset).astype(np.float32)


def _case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    K, step = 256, 8
    scale, offset = 30.0, 40.0
    if name == "k3":
        K = 3
    if name == "step2":
        step = 2
    if name == "negative_large":
        scale, offset = 3.0e3, -1.0e4
    books = _books(rng, K, step, scale, offset)
    if name == "zero_range":
        books[:, :, 0] = np.float32(12.5)          # a dimension every codeword agrees on, in every sub-space
        books[3, :, :] = books[3, 0, :]            # and a whole sub-space of equal codewords
    if name == "outlier":
        books[5, 17, :] *= np.float32(1000.0)      # one codeword stretches its sub-space's ranges
    codes = rng.integers(0, K, size=(ROWS, M)).astype(np.uint8)
    if name == "equal_rows":
        codes[:] = codes[0]
    if name == "outlier":
        codes[::7, 5] = 17
    # queries near the decoded rows, as real ones are
    dec = books[np.arange(M)[None, :], codes[:NQ]].reshape(NQ, M * step)
    q = (dec + rng.standard_normal(dec.shape).astype(np.float32) * np.float32(0.3 * scale)).astype(np.float32)
    if name == "big_query":
        q[4] *= np.float32(100.0)                  # makes the call's one scale coarse for everybody
    return books, codes, q


CASES = ["plain", "zero_range", "outlier", "big_query", "equal_rows", "k3", "negative_large", "step2"]


@pytest.mark.parametrize("name", CASES)
def test_bound_holds_for_every_pair(orc, name):
    books, codes, q = _case(name)
    im = IndexModel(books)
    assert im.ok, name
    X, n_hat = im.rows(codes)
    b = Batch(im, q)                               # (no coarse centroid: the residual is the query)
    assert b.usable and b.answerable.all(), name
    a = b.scores(X, n_hat)
    est = b.estimate(a)
    worst = 0.0
    for f in range(q.shape[0]):
        d_ref = orc.adc_scan(orc.lut(q[f], None, books), codes).astype(np.float64)
        err = np.abs(d_ref - est[f])
        worst = max(worst, float((err / b.E[f]).max()))
        assert (err <= b.E[f]).all(), (name, f, float(err.max()), float(b.E[f]))
    print("%s: worst |d_ref - estimate| / E_q = %.4f, t = %.4g" % (name, worst, b.t))
    # the integers stay where the kernels keep them
    assert np.abs(a).max() < 2 ** 29 and np.abs(b.W).max() <= 127 and np.abs(X).max() <= 127


def test_nonfinite_inputs_are_refused():
    books, codes, q = _case("plain")
    bad = books.copy(); bad[2, 9, 1] = np.inf
    assert not IndexModel(bad).ok
    im = IndexModel(books)
    q[3, 5] = np.nan
    b = Batch(im, q)
    assert b.usable and not b.answerable[3] and b.answerable[[0, 1, 2, 4]].all()
    zero = Batch(im, np.zeros_like(q))
    assert not zero.usable                          # t = 0: the call goes to the scan
