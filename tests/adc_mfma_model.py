"""A numpy restatement of the int8 matrix-core bound filter of large ADC batches (cvt_amd/csrc/adc_mfma.hip):
the per-index model, the decoded int8 rows, the query quantisation and the error bound E_q, formula for formula.

An ADC sum is the squared distance of the query residual r to the decoded row x^:  |r - x^|^2 = |r|^2 + |x^|^2 - 2 r.x^.
With x^ = c + s (.) (X + e), w = r (.) s = t (W + delta) and |x^|^2 = 2 t B + rho:

    d = C_q - 2 t a + rho - 2 t delta.X - 2 w.e,        a = W.X - B,   C_q = |r|^2 - 2 r.c

so |d_ref - (C_q - 2 t a)| <= E_q = 2 (t |delta| X_max + |w| eps_max) + 4 t + fp."""
import numpy as np

UP = 1.0 + 1e-9
BMAX = 4194304.0


def f32_up(x):
    """the smallest float32 >= x (x: float64 array)"""
    f = np.asarray(x, np.float64).astype(np.float32)
    low = f.astype(np.float64) < x
    return np.where(low, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


class IndexModel:
    """per index, from the codebooks [M][K][step] alone"""

    def __init__(self, books):
        books = np.asarray(books, np.float32)
        self.M, self.K, self.step = books.shape
        self.D = self.M * self.step
        b = books.astype(np.float64)
        self.ok = bool(np.isfinite(b).all())
        if not self.ok:
            return
        lo, hi = b.min(axis=1), b.max(axis=1)                      # [M][step]
        rng = hi - lo
        c = (0.5 * hi + 0.5 * lo).astype(np.float32)
        s = (rng / 254.0).astype(np.float32)
        c = np.where(rng == 0.0, lo.astype(np.float32), c)
        s = np.where(rng == 0.0, np.float32(0.0), s)
        if ((rng > 0) & ~(s >= np.finfo(np.float32).tiny)).any() or not (np.isfinite(c).all() and np.isfinite(s).all()):
            self.ok = False
            return
        self.c, self.s = c.reshape(-1), s.reshape(-1)              # [D]
        c64, s64 = c.astype(np.float64)[:, None, :], s.astype(np.float64)[:, None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.where(s64 > 0, (b - c64) / np.where(s64 > 0, s64, 1.0), 0.0)
        X = np.clip(np.rint(u), -127, 127)
        e = u - X
        self.Xb = X.astype(np.int64)                               # [M][K][step]
        self.nrm = (b * b).sum(axis=2)                             # [M][K]
        self.x_max = float(np.sqrt((X * X).sum(axis=2).max(axis=1).sum())) * UP
        self.eps_max = float(np.sqrt((e * e).sum(axis=2).max(axis=1).sum())) * UP + 1e-12
        self.xhat_max = float(np.sqrt(self.nrm.max(axis=1).sum())) * UP
        self.gamma = (self.step + 24) * 2.0 ** -24 * 1.01

    def rows(self, codes):
        """codes [n][M] -> (X [n][D] int64, n^ [n] float32 rounded up)"""
        codes = np.asarray(codes)
        m = np.arange(self.M)[None, :]
        X = self.Xb[m, codes].reshape(codes.shape[0], self.D)
        return X, f32_up(self.nrm[m, codes].sum(axis=1) * (1.0 + 1e-12))


class Batch:
    """per call: residuals r [nq][D] float32 (rotated query minus the centroid, as the reference's tables take it)"""

    def __init__(self, im, r):
        r = np.asarray(r, np.float32)
        self.finite = np.isfinite(r).all(axis=1)
        r64 = np.where(self.finite[:, None], r.astype(np.float64), 0.0)
        w = r64 * im.s.astype(np.float64)[None, :]
        wmax = f32_up(np.abs(w)).max() if self.finite.any() else np.float32(0.0)
        self.t = t = float(wmax) / 127.0 * (1.0 + 1e-12)
        self.usable = bool(t > 0.0 and np.isfinite(t) and im.xhat_max ** 2 * (1.0 + 1e-6) <= BMAX * 2.0 * t)
        if not self.usable:
            return
        u = w / t
        W = np.clip(np.rint(u), -127, 127)
        delta = u - W
        self.W = W.astype(np.int64)
        reach = np.sqrt((r64 * r64).sum(axis=1)) * UP + im.xhat_max
        fp = im.gamma * reach * reach + 1e-30
        self.E = (2.0 * (t * (np.sqrt((delta * delta).sum(axis=1)) * UP + 1e-9) * im.x_max + np.sqrt((w * w).sum(axis=1)) * UP * im.eps_max)
                  + 4.0 * t + fp) * UP
        self.C = (r64 * r64).sum(axis=1) - 2.0 * (r64 * im.c.astype(np.float64)[None, :]).sum(axis=1)
        self.margin = np.ceil(self.E / t) + 1.0
        self.answerable = self.finite & (self.margin < 268435456.0) & (reach * reach < 1e37)

    def scores(self, X, n_hat):
        """a [nq][n] = W.X - floor(n^ / 2t), exact integers"""
        B = np.floor(n_hat.astype(np.float64) / (2.0 * self.t)).astype(np.int64)
        return self.W @ X.T - B[None, :]

    def estimate(self, a):
        return self.C[:, None] - 2.0 * self.t * a.astype(np.float64)
