"""What test_gpu_sq8_routes.py rests on, none of it needing a GPU:

1. a host copy of the SQ8 dispatch (cvt_amd/csrc/sq8.hip: launch_sq8_train, launch_sq8_encode_rows with launch_sq8_encode_wave /
   launch_sq8_encode_group / sq8_group_blocks / launch_sq8_tile / launch_sq8_rownorm / launch_sq8_encode, and launch_sq8_decode): from
   the width, the row count, the normalisation flag, the alignment of the four pointers and the four tuning values to the ordered
   list of launches (name, grid, block, dynamic LDS) that cvt_amd.launch_log() must show;
2. a numpy restatement of the arithmetic, one fp32 (or fp64) operation per step, as a second opinion on the oracle's
   "restated only" quantise / decode loops (oracle/cvt_oracle.c: orc_sq8_*);
3. the tables and the hand-made ranges every case uses, and the list of cases itself.

Tables.  Rows come in a fixed order so that a table of any height holds a prefix of them (row 0 alone at n = 1):
  0 a row whose elements span 40 binades; 1 a row of -0.0; 2 a row whose sum of squares sits on a rounding boundary of the float
  root (the kernels cannot prove its norm from an unordered sum and replay it in index order; d >= 16); 3 a row x 1e30 (the fp32
  squares overflow, the norm is infinite, every quotient a signed zero); 4 a zero row; 5 a row x 1e-30; 6 a row with a single inf;
  7 .. 14 rows whose first eight columns are -0.0; 15 .. 214 the other 199 rows spanning 40 binades.
The last four columns are: d - 1 constant; d - 2 non-negative (its minimum is zero, with zeros of both signs, the first of them --
row 1 -- negative); d - 3 and d - 4, where a case asks for it, a maximum / a minimum that only the row `place` holds (in the sample
rows 0 .. 8191, at row 8192, or in the last row): the special rows are zero there, and `only_extreme` checks the claim."""
import math

import numpy as np

KB = 256                       # kBlock
SAMPLE_ROWS = 8192             # SQ8_SAMPLE_ROWS
TUNE_DEFAULT = dict(sq8_filter=1, sq8_encode_wave=1, sq8_flags=1, sq8_wave_blocks=3)

INIT, FINISH, ZFIRST, ZSIGN = "sq8_train_init_kernel", "sq8_train_finish_kernel", "sq8_zero_first_kernel", "sq8_zero_sign_kernel"
TILE, ROWNORM, TRAIN2, ENCODE2 = "sq8_tile_kernel", "sq8_rownorm_kernel", "sq8_train_kernel", "sq8_encode_kernel"
TRAIN_WF, TRAIN_W, TRAIN_G = "sq8_train_wave_f_kernel", "sq8_train_wave_kernel", "sq8_train_group_f_kernel"
ENC_WF, ENC_W, ENC_G = "sq8_encode_wave_f_kernel", "sq8_encode_wave_kernel", "sq8_encode_group_f_kernel"
DEC_LUT, DEC_VEC, DEC_ANY = "sq8_decode_lut_kernel", "sq8_decode_kernel", "sq8_decode_any_kernel"


# ---- 1. the dispatch ----

def blocks_for(count, per):
    return -(-count // per)


def wave_width(d):
    return d in (256, 512, 768, 1024, 1536, 2048)


def tile_ok(d, ax, ac, am, ad):
    return 4 <= d <= 512 and d % 4 == 0 and ax and ac and am and ad


def tile_launch(n, d):
    lds = 64 * ((d >> 2) + 1) * 16
    return (TILE, (min(256 if lds > 72 * 1024 else 512, blocks_for(n, 64)), 1, 1), 1024, lds)


def group_blocks(n, d, wb):
    return max(1, min(blocks_for((n * d + 255) // 256, KB // 64), 256 * wb))


def train_launches(d, n, l2norm, ax, tune=TUNE_DEFAULT):
    """launch_sq8_train; ax: x is 16-byte aligned"""
    filt, wb, db = tune["sq8_filter"] != 0, tune["sq8_wave_blocks"], blocks_for(d, KB)
    out = [(INIT, (db, 1, 1), KB, 0)]
    if n > 0:
        wave_f = filt and wave_width(d)
        ns = SAMPLE_ROWS if n >= 8 * SAMPLE_ROWS else 0
        if filt and d in (64, 128) and ax and n >= 4096:
            if ns:
                out.append((TRAIN_G, (group_blocks(ns // 16, d, wb), 1, 1), KB, 0))
            out.append((TRAIN_G, (group_blocks(n - ns, d, wb), 1, 1), KB, 0))
        elif (wave_f or (l2norm and d in (256, 512))) and ax and n >= (1 if wave_f and d > 512 else 4096):
            blocks = min(blocks_for(n, KB // 64), 256 * wb)
            if wave_f:
                if ns:
                    out.append((TRAIN_WF, (blocks_for(ns // 16, KB // 64), 1, 1), KB, 0))
                out.append((TRAIN_WF, (blocks, 1, 1), KB, 0))
            else:
                out.append((TRAIN_W, (blocks, 1, 1), KB, 0))
        elif tile_ok(d, ax, True, True, True):
            out.append(tile_launch(n, d))
        else:
            if l2norm:
                out.append((ROWNORM, (blocks_for(n, 64), 1, 1), KB, 0))
            out.append((TRAIN2, (blocks_for(n, 512), 1, 1), KB, 0))
    out.append((FINISH, (db, 1, 1), KB, 0))
    if 0 < n < 0xffffffff:
        out.append((ZFIRST, (min(blocks_for(n, KB), 1024), 1, 1), KB, 0))
        out.append((ZSIGN, (db, 1, 1), KB, 0))
    return out


def encode_launches(d, n, l2norm, ax, ac, am, ad, tune=TUNE_DEFAULT):
    """launch_sq8_encode_rows; l2norm 0 / 1 / 2 as the C entry takes it; the bits: x / vmin / vdiff 16-byte, codes 4-byte aligned"""
    if n <= 0:
        return []
    filt, ew, wb = tune["sq8_filter"] != 0, tune["sq8_encode_wave"] != 0, tune["sq8_wave_blocks"]
    aligned = ax and ac and am and ad
    if ew and filt and d in (64, 128) and n >= 4096 and aligned:
        return [(ENC_G, (group_blocks(n, d, wb), 1, 1), KB, 0)]
    if ew and wave_width(d) and n >= (1 if d > 512 else 4096) and aligned and (d <= 512 or filt):
        return [(ENC_WF if filt else ENC_W, (min(blocks_for(n, KB // 64), 256 * wb), 1, 1), KB, 0)]
    if tile_ok(d, ax, ac, am, ad):
        return [tile_launch(n, d)]
    out = [(ROWNORM, (blocks_for(n, 64), 1, 1), KB, 0)] if l2norm else []
    return out + [(ENCODE2, (min(blocks_for(n, 16), 4096), 1, 1), KB, 0)]


def decode_split(d, n):
    """(slabs, row_splits) of the table kernel"""
    slabs = blocks_for(d, 128)
    rs = blocks_for(256, slabs)
    if rs * 2048 > n:
        rs = max(1, n // 2048)
    return slabs, rs


def decode_launches(d, n, ax, ac, am, ad):
    """launch_sq8_decode (both arithmetic modes take the same route); ax: the OUTPUT rows"""
    if n <= 0:
        return []
    if d % 4 == 0 and ax and ac and n >= 16384:
        slabs, rs = decode_split(d, n)
        return [(DEC_LUT, (slabs * rs, 1, 1), 512, 4 * 256 * 32 * 4)]
    vec = d % 4 == 0 and ax and ac and am and ad
    return [(DEC_VEC if vec else DEC_ANY, (min(blocks_for(n, 16), 4096), 1, 1), KB, 0)]


def wave_rows_in_flight(d):
    """RB of the filter kernels: rows a wave holds per step"""
    nf = d // 256
    return 4 if nf <= 2 else 2 if nf <= 4 else 1


# ---- 2. the arithmetic, restated ----

F32 = np.float32


def norms(x, chunk=4096):
    """fp32 [n]: float(max(1e-12, sqrt(sum))) with sum the float64 running sum, in index order, of the fp32 products"""
    n = x.shape[0]
    den = np.empty(n, F32)
    with np.errstate(all="ignore"):
        for r0 in range(0, n, chunk):
            sq = x[r0:r0 + chunk] * x[r0:r0 + chunk]
            assert sq.dtype == F32
            s = np.add.accumulate(sq.astype(np.float64), axis=1)[:, -1]      # sequential: one addition after the other
            root = np.sqrt(s)
            den[r0:r0 + chunk] = np.where(root > 1e-12, root, 1e-12).astype(F32)
    return den


def unproven(x):
    """bool [n]: rows whose float root the kernels cannot take from an unordered sum (the roots of sum (1 -+ 2^-42) differ)"""
    with np.errstate(all="ignore"):
        s = np.add.accumulate((x * x).astype(np.float64), axis=1)[:, -1]
        lo, hi = np.sqrt(s * (1.0 - 2.0 ** -42)), np.sqrt(s * (1.0 + 2.0 ** -42))
        return ~(np.where(lo > 1e-12, lo, 1e-12).astype(F32) == np.where(hi > 1e-12, hi, 1e-12).astype(F32))


def normalised(x, l2norm):
    if not l2norm:
        return x
    with np.errstate(all="ignore"):
        a = x / norms(x)[:, None]
    assert a.dtype == F32
    return a


def encode(vmin, vdiff, x, l2norm):
    """(codes uint8 [n][d], rows after the call); the code of a NaN is whatever the conversion gives: callers exclude it"""
    a = normalised(x, l2norm)
    with np.errstate(all="ignore"):
        b = a - vmin[None, :]
        xi = b / vdiff[None, :]
        xi = np.where((vdiff != 0)[None, :], xi, F32(0))
        xi = np.where(xi < 0, F32(0), xi)
        xi = np.where(xi > 1, F32(1), xi)
        y = F32(255) * xi
        assert y.dtype == F32
        codes = np.nan_to_num(y, nan=0.0).astype(np.int32).astype(np.uint8)
    return codes, a


def decode(vmin, vdiff, codes, mode):
    with np.errstate(all="ignore"):
        if mode == 0:
            t = vdiff.astype(np.float64)[None, :] * (codes.astype(np.float64) + 0.5)
            return (vmin.astype(np.float64)[None, :] + t / 255.0).astype(F32)
        xi = (codes.astype(F32) + F32(0.5)) / F32(255)
        prod = xi * vdiff[None, :]
        out = vmin[None, :] + prod
    assert out.dtype == F32
    return out


def train(x, l2norm):
    """(vmin, vdiff): the first smallest / largest element of every column in row order (strict comparisons: NaN never enters,
    of two zeros the first stays), then max - min"""
    a = normalised(x, l2norm)
    cols = np.arange(a.shape[1])
    with np.errstate(all="ignore"):
        def first(red, empty):
            m = red.reduce(a, axis=0) if a.shape[0] else np.full(a.shape[1], np.nan, F32)
            eq = a == m[None, :]
            hit = eq.any(axis=0)
            return np.where(hit, a[np.argmax(eq, axis=0), cols] if a.shape[0] else m, F32(empty)).astype(F32)
        lo, hi = first(np.fmin, np.inf), first(np.fmax, -np.inf)
        return lo, hi - lo


# ---- 3. tables, ranges, cases ----

N_SPECIAL = 215


def boundary_row(d):
    """a row whose squares are exact in fp32 and add up, in any order and together with the 0.25 of the constant column, to within
    2^-46 of (1 + 99 * 2^-24)^2: the square of the midpoint between two floats, so that the float roots of sum (1 -+ 2^-42) differ"""
    r = ((1 << 24) + 99) ** 2 - (1 << 44)           # in units of 2^-48; 2^44 = 0.25^2
    vals = []
    while r >= 4:
        q = math.isqrt(r)
        s = max(0, q.bit_length() - 12)
        a = q >> s                                  # 12 bits: a^2 is exact in fp32
        vals.append(math.ldexp(a, s - 24))
        r -= (a << s) ** 2
    assert len(vals) <= 12
    row = np.zeros(d, F32)
    if d >= 16:
        row[np.arange(len(vals)) * ((d - 4) // len(vals))] = vals      # spread over the lanes, clear of the last four columns
    return row


def place_row(n, place):
    if place is None:
        return None
    if place == "sample":
        return 4000 if n > SAMPLE_ROWS else n // 2
    if place == "8192":
        assert n > SAMPLE_ROWS
        return SAMPLE_ROWS
    return n - 1


def table(d, n, place=None):
    """the rows of one case (module docstring); deterministic in (d, n, place)"""
    rng = np.random.default_rng(d * 1_000_003 + n)
    x = rng.standard_normal(size=(n, d), dtype=F32)
    wide = np.exp2(rng.integers(-20, 21, size=(N_SPECIAL, d))).astype(F32)
    for i in [0] + list(range(15, N_SPECIAL)):
        if i < n:
            x[i] *= wide[i]
    if n > 1:
        x[1] = F32(-0.0)
    if n > 2 and d >= 16:
        x[2] = boundary_row(d)
    if n > 3:
        x[3] *= F32(1e30)
    if n > 4:
        x[4] = F32(0.0)
    if n > 5:
        x[5] *= F32(1e-30)
    if n > 6:
        x[6, d // 2] = np.inf
    if n > 7:
        x[7:15, :max(1, min(8, d - 4))] = F32(-0.0)
    if d >= 4:
        x[:, d - 1] = F32(0.25)
        x[:, d - 2] = np.abs(x[:, d - 2])
        if n > 1:
            x[1, d - 2] = F32(-0.0)
    pr = place_row(n, place)
    if pr is not None:
        assert d >= 64 and pr >= N_SPECIAL
        x[:N_SPECIAL, d - 4:d - 2] = 0
        x[pr, d - 3] = F32(1000.0)
        x[pr, d - 4] = F32(-1000.0)
    return x


def only_extreme(x, place, l2norm):
    """the row `place` holds the strict maximum of column d - 3 and the strict minimum of column d - 4 of the (normalised) rows"""
    n, d = x.shape
    pr = place_row(n, place)
    a = normalised(x[:, d - 4:d - 2], False)
    if l2norm:
        with np.errstate(all="ignore"):
            a = a / norms(x)[:, None]
    rest = np.delete(a, pr, axis=0)
    return bool(a[pr, 1] > np.nanmax(rest[:, 1]) and a[pr, 0] < np.nanmin(rest[:, 0]))


def training_rows(x):
    """the rows the hand-made ranges are trained on: finite, and without the special rows where the table has others"""
    n = x.shape[0]
    keep = np.all(np.isfinite(x), axis=1)
    if n > N_SPECIAL + 16:
        keep[:N_SPECIAL] = False
    else:
        keep[3:7] = False
    return x[keep]


def hand_made(vmin, vdiff):
    """the ranges of test_sq8_decision_filter_equals_the_chain: vdiff 0 / 1e-41 / 1e30 / NaN / negative, |vmin| >> vdiff, a -0.0
    minimum, and a range narrower than the data on either side (both clamps act)"""
    hv, hd = vmin.copy(), vdiff.copy()
    d = hv.shape[0]
    edits = [(1, None, 0.0), (2, None, 1e-41), (3, None, 1e30), (4, 50.0, 1e-3), (5, None, np.nan), (6, -0.0, None)]
    for c, v, df in edits:
        if c < d:
            if v is not None:
                hv[c] = v
            if df is not None:
                hd[c] = df
    if d > 7:
        hd[7] = -abs(hd[7])
    if d > 8:
        hv[8] = hv[8] + F32(0.3) * hd[8]
    if d > 9:
        hd[9] *= F32(0.4)
    return hv, hd


DIFF_SPECIALS = [0.0, 1e-41, 2.0 ** -101, 2.0 ** -100, 2.0 ** 100, 2.0 ** 101, -0.37]


def decode_inputs(d, n):
    """(vmin, vdiff, codes): every byte value in every column (n >= 256), the rest random; vdiff 0, a denormal, 2^-101 | 2^-100 and
    2^100 | 2^101 (either side of the kernels' guard for the reciprocal of 255) and a negative one, rotated by n so that the narrowest
    table meets all of them over its row counts, and once more in the last columns"""
    rng = np.random.default_rng(d * 7919 + n)
    vmin = rng.standard_normal(size=d, dtype=F32)
    vdiff = (np.abs(rng.standard_normal(size=d, dtype=F32)) * F32(0.01) + F32(1e-3)).astype(F32)
    k = len(DIFF_SPECIALS)
    for c in range(min(d, k)):
        vdiff[c] = F32(DIFF_SPECIALS[(c + n) % k])
    if d >= 2 * k:
        vdiff[d - k:] = np.float32(DIFF_SPECIALS)
    codes = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    m = min(n, 256)
    codes[:m] = ((np.arange(m)[:, None] + 37 * np.arange(d)[None, :]) & 255).astype(np.uint8)
    return vmin, vdiff, codes


# The cases.  (d, n, place, tuning overrides, the kernels the shape is there for: train, encode)
def T(**kw):
    return dict(TUNE_DEFAULT, **kw)


GROUP = [(d, n) for d in (64, 128) for n in (4095, 4096, 4097, 4099)]
SAMPLE_SWITCH = [(d, n, place) for d in (64, 128, 256, 768) for n, place in ((65_535, "last"), (65_536, "sample"), (65_537, "8192"))]
WAVE_MID = [(d, n) for d in (256, 512) for n in (4095, 4096, 4101)]
WAVE_WIDE = [(d, n) for d in (768, 1024, 1536, 2048) for n in (1, 2, 3, 5, 17, 1031)]
CHAIN = [(d, n) for d in (256, 512) for n in (4096, 4101)]
TILE_SMALL = [(d, n) for d in (4, 12, 508, 512) for n in (1, 63, 64, 65)]
TILE_LOOP = [(64, 64 * 512 + 65), (512, 64 * 256 + 65)]
TWO_PASS = [(d, n) for d in (7, 257, 516) for n in (15, 16, 17, 63, 64, 65, 511, 512, 513)]
TWO_PASS_LOOP = (7, 65_536 + 17)
MISALIGNED = [(64, 4101), (512, 4101), (1024, 1031)]
DECODE_TABLE = [(d, 16_385) for d in (4, 124, 128, 132, 260, 516, 2048)] + [(d, n) for d in (4, 132) for n in (16_383, 16_384)] + [(2048, 32_769)]
DECODE_ANY = [(5, 100), (5, 16_385)]


def all_tables():
    """(d, n, place) of every table a GPU case trains or encodes"""
    keys = [(d, n, None) for d, n in GROUP + WAVE_MID + WAVE_WIDE + CHAIN + TILE_SMALL + TILE_LOOP + TWO_PASS + [TWO_PASS_LOOP] + MISALIGNED]
    keys += SAMPLE_SWITCH + [(512, 5000, None), (1024, 17, None), (64, 65_536, "sample"), (256, 65_536, "sample")]
    return sorted(set(keys), key=lambda k: (k[0], k[1], str(k[2])))
