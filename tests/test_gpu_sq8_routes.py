"""The SQ8 train, encode and decode kernels by name (cvt_amd/csrc/sq8.hip): 17 kernels behind cvtmi_sq8_train, cvtmi_sq8_encode and
cvtmi_sq8_decode / _decode_faiss, picked by row width, row count, pointer alignment and four tuning keys.  Every GPU case runs inside
cvt_amd.launch_log() and asserts that the log EQUALS the list a host copy of the dispatch expects (sq8_routes_model.py: name, grid,
block, dynamic LDS, in order -- so no other kernel ran), with the alignment bits read off the pointers that were passed, and that the
kernel the shape is there for is in that list.  test_cases_reach_their_kernels makes the second claim without a GPU.

Results are compared with the oracle bit for bit: vmin / vdiff by bit pattern (the sign of a zero minimum included), codes with
array_equal, written-back and decoded rows by bit pattern.  Excluded, as in test_gpu_flat_sq8.py and for its reason -- (int) NaN is
undefined in the reference itself -- are the code bytes of rows that hold a non-finite value after normalisation and of columns whose
vdiff is not finite; every case asserts that these are at most 3 rows and 2 columns.  The oracle's quantise / decode loops are restated
from the reference's text, so test_restatement_equals_the_oracle checks them, without a GPU, against a numpy restatement with one
operation per step on every table the GPU cases use.

What each table holds, and where a case puts a column's only extreme, is in sq8_routes_model.py."""
import contextlib
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import sq8_routes_model as M
from conftest import bits
from sq8_routes_model import T

gpu = pytest.mark.gpu
KEYS = tuple(M.TUNE_DEFAULT)


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import cvt_amd
    cvt_amd.lib()
    return cvt_amd


# ---- the cases: which tuning settings a shape runs under, and the kernel it is there for ----

def wave_block_variants(base):
    return [dict(base, sq8_wave_blocks=1), dict(base, sq8_wave_blocks=64)]


def tunes_for(family, d, n):
    if family in ("group", "sample"):
        return [T()] + wave_block_variants(T()) + ([T(sq8_flags=0)] if d >= 256 else [])
    if family in ("wave_mid", "wave_wide"):
        return [T(), T(sq8_flags=0)] + (wave_block_variants(T()) if n in (4101, 1031) else [])
    if family == "chain":
        return [T(sq8_filter=0)] + (wave_block_variants(T(sq8_filter=0)) if n == 4101 else [])
    if family == "tile_loop":
        return [T(sq8_filter=0, sq8_encode_wave=0)]
    if family == "tile_nowave":
        return [T(sq8_encode_wave=0)]
    if family == "wide_filter_off":
        return [T(sq8_filter=0)]
    return [T()]                                   # tile, two_pass, misaligned


def want(family, d, n, l2norm):
    """(training kernel, encode kernel) the case is there for; None: the shape is not about that entry"""
    if family in ("group", "sample") and d in (64, 128):
        return (M.TRAIN_G, M.ENC_G) if n >= 4096 else (M.TILE, M.TILE)
    if family in ("wave_mid", "wave_wide", "sample"):
        return (M.TRAIN_WF, M.ENC_WF) if n >= 4096 or d > 512 else (M.TILE, M.TILE)
    if family == "chain":
        return (M.TRAIN_W if l2norm else M.TILE, M.ENC_W)
    if family == "tile_loop":
        return (M.TRAIN_W if l2norm and d == 512 else M.TILE, M.TILE)
    if family == "tile_nowave":
        return (None, M.TILE)
    if family == "tile":
        return (M.TILE, M.TILE)
    return (M.TRAIN2, M.ENCODE2)                   # two_pass, wide_filter_off, misaligned


FAMILIES = {"group": M.GROUP, "wave_mid": M.WAVE_MID, "wave_wide": M.WAVE_WIDE, "chain": M.CHAIN, "tile": M.TILE_SMALL, "tile_loop": M.TILE_LOOP,
            "tile_nowave": [(512, 5000)], "two_pass": M.TWO_PASS + [M.TWO_PASS_LOOP], "wide_filter_off": [(1024, 17)]}
MISALIGN = ("x", "codes", "vmin")
HOST = [(64, 4097), (256, 4101), (1024, 5), (12, 65), (257, 65)]


def planned_routes():
    """every list of launches the GPU cases below expect, by the host copy of the dispatch"""
    out = []
    for family, shapes in FAMILIES.items():
        for d, n in shapes:
            for tune in tunes_for(family, d, n):
                out += [M.train_launches(d, n, l2, True, tune) for l2 in (1, 0)]
                out += [M.encode_launches(d, n, l2, True, True, True, True, tune) for l2 in (1, 2, 0)]
    for d, n, _ in M.SAMPLE_SWITCH:
        for tune in tunes_for("sample", d, n):
            out += [M.train_launches(d, n, l2, True, tune) for l2 in (1, 0)]
    for d, n in M.MISALIGNED:
        out += [M.train_launches(d, n, l2, False, T()) for l2 in (1, 0)]
        for which in MISALIGN:
            out += [M.encode_launches(d, n, l2, which != "x", which != "codes", which != "vmin", True, T()) for l2 in (1, 2, 0)]
    out += [M.decode_launches(d, n, True, True, True, True) for d, n in M.DECODE_TABLE + M.DECODE_ANY]
    out += [M.decode_launches(128, 16_385, False, True, True, True), M.decode_launches(128, 16_383, True, True, False, True)]
    return out


# ---- CPU: the cases against the dispatch, the sources against the cases, the restatement against the oracle ----

def test_cases_reach_their_kernels():
    """host logic: by the copy of the dispatch, every shape takes the kernel it is listed for under every tuning setting it runs with
    (and the rows one short of a threshold do not), and the cases together launch every template family the file holds"""
    for family, shapes in FAMILIES.items():
        for d, n in shapes:
            for tune in tunes_for(family, d, n):
                for l2 in (1, 0):
                    wt, we = want(family, d, n, l2)
                    names = [r[0] for r in M.train_launches(d, n, l2, True, tune)]
                    assert wt is None or wt in names, (family, d, n, l2, tune, names)
                    assert names[0] == M.INIT and names[-3:] == [M.FINISH, M.ZFIRST, M.ZSIGN]
                    names = [r[0] for r in M.encode_launches(d, n, l2, True, True, True, True, tune)]
                    assert we in names, (family, d, n, l2, tune, names)
    for d, n in M.GROUP + M.WAVE_MID:
        if n == 4095:
            assert want("group" if d <= 128 else "wave_mid", d, n, 1) == (M.TILE, M.TILE)
    for d, n, _ in M.SAMPLE_SWITCH:
        for l2 in (1, 0):
            names = [r[0] for r in M.train_launches(d, n, l2, True, T())]
            assert names.count(want("sample", d, n, l2)[0]) == (2 if n >= 65_536 else 1), (d, n, names)
    for d, n in M.MISALIGNED:
        for l2 in (1, 0):
            assert M.TRAIN2 in [r[0] for r in M.train_launches(d, n, l2, False, T())]
            assert M.TRAIN2 not in [r[0] for r in M.train_launches(d, n, l2, True, T())]
            for which in MISALIGN:
                names = [r[0] for r in M.encode_launches(d, n, l2, which != "x", which != "codes", which != "vmin", True, T())]
                assert names == ([M.ROWNORM] if l2 else []) + [M.ENCODE2]
    for d, n in M.DECODE_TABLE:
        assert [r[0] for r in M.decode_launches(d, n, True, True, True, True)] == [M.DEC_LUT if n >= 16_384 else M.DEC_VEC]
    for d, n in M.DECODE_ANY:
        assert [r[0] for r in M.decode_launches(d, n, True, True, True, True)] == [M.DEC_ANY]
    assert M.decode_split(2048, 32_769) == (16, 16) and M.decode_split(2048, 16_385) == (16, 8) and M.decode_split(132, 16_385) == (2, 8)
    # the looping tile: more tiles than the grid cap
    for d, n in M.TILE_LOOP:
        grid = M.tile_launch(n, d)[1][0]
        assert grid == (512 if d == 64 else 256) and M.blocks_for(n, 64) > grid
    assert M.blocks_for(M.TWO_PASS_LOOP[1], 16) > 4096
    # every filter instance: NF = d / 256 in 1, 2, 3, 4, 6, 8 (x NORM by the l2norm loop), 16 and 32 lanes per row
    assert {d // 256 for d, _ in M.WAVE_MID + M.WAVE_WIDE} == {1, 2, 3, 4, 6, 8}
    # rows in flight: n = 4101 / 1031 are no multiple of RB x waves under either grid
    for d, n in [(256, 4101), (512, 4101)] + [(d, 1031) for d in (768, 1024, 1536, 2048)]:
        for wb in (1, 3, 64):
            waves = 4 * min(M.blocks_for(n, 4), 256 * wb)
            assert n % (M.wave_rows_in_flight(d) * waves) != 0


def test_every_launch_name_is_expected():
    """every kernel name sq8.hip passes to launch( / launch_lds( is expected by at least one case: a kernel added later fails here
    instead of going untested"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cvt_amd", "csrc", "sq8.hip")
    with open(src) as f:
        launched = set(re.findall(r'\blaunch(?:_lds)?\(\s*"([A-Za-z0-9_]+)"', f.read()))
    assert len(launched) >= 17, sorted(launched)
    expected = {r[0] for route in planned_routes() for r in route}
    assert launched <= expected, sorted(launched - expected)
    assert expected <= launched, sorted(expected - launched)


@functools.lru_cache(maxsize=2)
def table(d, n, place):
    x = M.table(d, n, place)
    x.flags.writeable = False
    return x


_ref = {}


def oracle_train(orc, key, l2norm):
    k = ("train", key, bool(l2norm))
    if k not in _ref:
        _ref[k] = orc.sq8_train(table(*key), l2norm=bool(l2norm))
    return _ref[k]


def ranges(orc, key, l2norm):
    """the hand-made ranges of one table (trained on its ordinary rows by the oracle)"""
    k = ("ranges", key, bool(l2norm))
    if k not in _ref:
        _ref[k] = M.hand_made(*orc.sq8_train(M.training_rows(table(*key)), l2norm=bool(l2norm)))
    return _ref[k]


@functools.lru_cache(maxsize=4)
def _oracle_encode(orc, key, l2norm):
    hv, hd = ranges(orc, key, l2norm)
    return orc.sq8_encode(hv, hd, table(*key), l2norm=l2norm)


def oracle_encode(orc, key, l2norm):
    return _oracle_encode(orc, key, bool(l2norm))


def comparable(x, ox, hd):
    """(rows, columns) whose code bytes the reference defines; at most 3 rows and 2 columns are left out"""
    fin, fin_cols = np.all(np.isfinite(ox), axis=1) & np.all(np.isfinite(x), axis=1), np.isfinite(hd)
    assert (~fin).sum() <= 3 and (~fin_cols).sum() <= 2, ((~fin).sum(), (~fin_cols).sum())
    return fin, fin_cols


@pytest.mark.parametrize("d,n,place", M.all_tables())
def test_restatement_equals_the_oracle(orc, d, n, place):
    """the numpy restatement (one fp32 operation per step; the norm a float64 running sum in index order) against the oracle's loops:
    trained ranges on the whole table, codes on the rows and columns the reference defines, normalised rows on the finite rows; and
    the table's own claims: row 2 needs the index-order replay, the placed extreme is the column's only one"""
    key = (d, n, place)
    x = table(*key)
    if n > 2 and d >= 16:
        assert M.unproven(x[:3])[2]
    for l2 in (True, False):
        ovm, ovd = oracle_train(orc, key, l2)
        mvm, mvd = M.train(x, l2)
        assert np.array_equal(bits(mvm), bits(ovm)) and np.array_equal(bits(mvd), bits(ovd)), (key, l2)
        if place is not None:
            assert M.only_extreme(x, place, l2)
            continue                                   # (the sample-switch tables are only trained on)
        hv, hd = ranges(orc, key, l2)
        oc, ox = oracle_encode(orc, key, l2)
        mc, mx = M.encode(hv, hd, x, l2)
        fin, fin_cols = comparable(x, ox, hd)
        assert np.array_equal(mc[fin][:, fin_cols], oc[fin][:, fin_cols]), (key, l2)
        assert np.array_equal(bits(mx[fin]), bits(ox[fin])), (key, l2)
        if n > 6 and l2:
            assert not fin[6] and fin.sum() == n - 1
    _oracle_encode.cache_clear()


@pytest.mark.parametrize("d,n", M.DECODE_TABLE + M.DECODE_ANY)
def test_decode_restatement_equals_the_oracle(orc, d, n):
    """mode 0: vmin + vdiff (b + 0.5) / 255 in float64, rounded once; mode 1: three fp32 roundings -- on the rows that hold every byte"""
    vmin, vdiff, codes = M.decode_inputs(d, n)
    codes = codes[:1024]
    if n >= 256:
        assert all(len(np.unique(codes[:, c])) == 256 for c in range(d))
    assert np.array_equal(bits(M.decode(vmin, vdiff, codes, 0)), bits(orc.sq8_decode(vmin, vdiff, codes)))
    assert np.array_equal(bits(M.decode(vmin, vdiff, codes, 1)), bits(orc.sq8_decode_faiss(vmin, vdiff, codes)))


# ---- GPU: running a case ----

@contextlib.contextmanager
def tuned(amd, tune):
    old = {name: amd.get_tuning(name) for name in KEYS}
    try:
        for name in KEYS:
            amd.set_tuning(name, tune[name])
        yield
    finally:
        for name, value in old.items():
            amd.set_tuning(name, value)


def dev_empty(shape, dtype, off=0):
    """a contiguous CUDA tensor `off` elements into a larger allocation (the allocation itself is aligned far beyond 16 bytes)"""
    import torch
    numel = int(np.prod(shape))
    buf = torch.empty(numel + 16, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf[off:off + numel].view(*shape)


def dev(a, off=0):
    import torch
    t = torch.from_numpy(np.array(a))          # (a copy: the shared tables are read-only)
    v = dev_empty(t.shape, t.dtype, off)
    v.copy_(t)
    return v


def al(t, by):
    return t.data_ptr() % by == 0


def ptr(t):
    assert t.is_contiguous()
    return C.c_void_p(t.data_ptr())


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def train_dev(amd, xt, l2norm, tune):
    """cvtmi_sq8_train_dev -> (vmin, vdiff, log, the list the dispatch copy expects)"""
    import torch
    n, d = xt.shape
    vmin, vdiff = dev_empty((d,), torch.float32), dev_empty((d,), torch.float32)
    with tuned(amd, tune), amd.launch_log() as log:
        rc = amd.lib().cvtmi_sq8_train_dev(ptr(xt), C.c_int64(n), C.c_int(d), C.c_int(l2norm), ptr(vmin), ptr(vdiff), stream())
    assert rc == 0
    return vmin.cpu().numpy(), vdiff.cpu().numpy(), log, M.train_launches(d, n, l2norm, al(xt, 16), tune)


def encode_dev(amd, vmin, vdiff, xt, l2norm, codes, tune):
    n, d = xt.shape
    with tuned(amd, tune), amd.launch_log() as log:
        rc = amd.lib().cvtmi_sq8_encode_dev(ptr(vmin), ptr(vdiff), C.c_int(d), ptr(xt), C.c_int64(n), C.c_int(l2norm), ptr(codes), stream())
    assert rc == 0
    return codes.cpu().numpy(), xt.cpu().numpy(), log, M.encode_launches(d, n, l2norm, al(xt, 16), al(codes, 4), al(vmin, 16), al(vdiff, 16), tune)


def names(log):
    return [r[0] for r in log]


def check_train(amd, orc, key, family, tunes, x_off=0, wanted=None):
    """both normalisation flags under every tuning setting: the log, vmin and vdiff bit for bit"""
    d, n, _ = key
    x = table(*key)
    xt = dev(x, x_off)
    for l2 in (1, 0):
        ovm, ovd = oracle_train(orc, key, l2)
        for tune in tunes:
            vm, vd, log, expect = train_dev(amd, xt, l2, tune)
            assert log == expect, (key, l2, tune, log, expect)
            wt = wanted if wanted is not None else want(family, d, n, l2)[0]
            assert wt is None or wt in names(log), (key, l2, tune, log)
            assert np.array_equal(bits(vm), bits(ovm)), (key, l2, tune, np.flatnonzero(bits(vm) != bits(ovm))[:8])
            assert np.array_equal(bits(vd), bits(ovd)), (key, l2, tune, np.flatnonzero(bits(vd) != bits(ovd))[:8])
    assert np.array_equal(bits(xt.cpu().numpy()), bits(x)), "training wrote to its rows"


def check_encode(amd, orc, key, family, tunes, off=(0, 0, 0), wanted=None):
    """l2norm 1 (rows normalised in place), 2 (normalised codes, rows left alone) and 0 under every tuning setting: the log, the
    codes, the rows; every setting must also give the same bytes everywhere, the rows and columns the reference leaves undefined included"""
    import torch
    d, n, _ = key
    x = table(*key)
    for l2 in (1, 2, 0):
        hv, hd = ranges(orc, key, l2)
        oc, ox = oracle_encode(orc, key, l2)
        fin, fin_cols = comparable(x, ox, hd)
        vm, vd = dev(hv, off[2]), dev(hd)
        first = None
        for tune in tunes:
            xt, ct = dev(x, off[0]), dev_empty((n, d), torch.uint8, off[1])
            ct.fill_(0xA5)
            codes, rows, log, expect = encode_dev(amd, vm, vd, xt, l2, ct, tune)
            assert log == expect, (key, l2, tune, log, expect)
            we = wanted if wanted is not None else want(family, d, n, l2)[1]
            assert we in names(log), (key, l2, tune, log)
            bad = np.flatnonzero(np.any(codes[:, fin_cols] != oc[:, fin_cols], axis=1) & fin)
            assert bad.size == 0, (key, l2, tune, "rows", bad[:8].tolist())
            assert np.array_equal(bits(rows), bits(ox if l2 == 1 else x)), (key, l2, tune)
            if first is None:
                first = codes
            assert np.array_equal(codes, first), (key, l2, tune, "tuning settings disagree")


def run_family(amd, orc, family, d, n):
    key, tunes = (d, n, None), tunes_for(family, d, n)
    check_train(amd, orc, key, family, tunes)
    check_encode(amd, orc, key, family, tunes)
    _oracle_encode.cache_clear()


# ---- GPU: the cases ----

@gpu
@pytest.mark.parametrize("d,n", M.GROUP)
def test_group_kernels(amd, orc, d, n):
    """sq8_train_group_f_kernel / sq8_encode_group_f_kernel, 16 and 32 lanes per row, NORM on and off: 4095 rows stay on the tile kernel,
    4096 / 4097 / 4099 rows (a last group of 1 .. 4 rows) take them; sq8_wave_blocks 1, 3 and 64 (64: more waves than groups)"""
    run_family(amd, orc, "group", d, n)


@gpu
@pytest.mark.parametrize("d,n,place", M.SAMPLE_SWITCH)
def test_sample_pass_switch(amd, orc, d, n, place):
    """training one row either side of 8 x 8192 rows: one launch at 65 535, the sample pass over rows 0 .. 8191 and the seeded pass at
    65 536 / 65 537; a column's only maximum and only minimum sit in the last row, in a sample row, in row 8192 (the first seeded row)"""
    key = (d, n, place)
    tunes = tunes_for("sample", d, n)
    check_train(amd, orc, key, "sample", tunes)
    for l2 in (1, 0):
        route = names(M.train_launches(d, n, l2, True, T()))
        assert route.count(want("sample", d, n, l2)[0]) == (2 if n >= 65_536 else 1)


@gpu
@pytest.mark.parametrize("d", [64, 256])
def test_sample_pass_changes_nothing(amd, orc, d):
    """rows 0 .. n - 1 trained at n = 65 535 (no sample pass) and at n = 65 536 (with it) differ only by what row 65 535 contributes:
    where its normalised value lies strictly inside the range of the rows before it, the two results have the same bits"""
    key = (d, 65_536, "sample")
    x = table(*key)
    xt = dev(x)
    for l2 in (1, 0):
        a = M.normalised(x, l2)
        with np.errstate(all="ignore"):
            lo, hi = np.fmin.reduce(a[:-1], axis=0), np.fmax.reduce(a[:-1], axis=0)
        inside = (a[-1] > lo) & (a[-1] < hi)
        assert inside.sum() >= d // 2
        vm0, vd0, log0, expect0 = train_dev(amd, xt[:-1], l2, T())
        vm1, vd1, log1, expect1 = train_dev(amd, xt, l2, T())
        assert log0 == expect0 and log1 == expect1 and len(log1) == len(log0) + 1, (log0, log1)
        ovm, ovd = oracle_train(orc, key, l2)
        assert np.array_equal(bits(vm1), bits(ovm)) and np.array_equal(bits(vd1), bits(ovd)), (d, l2)
        pvm, pvd = orc.sq8_train(x[:-1], l2norm=bool(l2))
        assert np.array_equal(bits(vm0), bits(pvm)) and np.array_equal(bits(vd0), bits(pvd)), (d, l2)
        assert np.array_equal(bits(vm0)[inside], bits(vm1)[inside]) and np.array_equal(bits(vd0)[inside], bits(vd1)[inside]), (d, l2)


@gpu
@pytest.mark.parametrize("d,n", M.WAVE_MID + M.WAVE_WIDE)
def test_wave_filter_kernels(amd, orc, d, n):
    """sq8_train_wave_f_kernel / sq8_encode_wave_f_kernel, NF = 1, 2, 3, 4, 6, 8 x NORM: d = 256 / 512 from 4096 rows (4095: the tile
    kernel), d = 768 .. 2048 from one row up -- fewer rows than waves, RB = 2 or 1 rows in flight, tail rows clamped to row n - 1;
    both wave-sum flavours (sq8_flags), and sq8_wave_blocks 1 and 64 at n = 4101 / 1031"""
    run_family(amd, orc, "wave_mid" if d <= 512 else "wave_wide", d, n)


@gpu
@pytest.mark.parametrize("d,n", M.CHAIN + [(1024, 17)])
def test_chain_kernels(amd, orc, d, n):
    """sq8_filter 0: sq8_train_wave_kernel (normalising training only) and sq8_encode_wave_kernel at d = 256 / 512; rows wider than
    512 floats go to the two-pass kernels"""
    run_family(amd, orc, "chain" if d <= 512 else "wide_filter_off", d, n)


@gpu
@pytest.mark.parametrize("d,n", M.TILE_SMALL + M.TILE_LOOP + [(512, 5000)])
def test_tile_kernel(amd, orc, d, n):
    """sq8_tile_kernel<TRAIN> and <false>: the narrowest and the widest rows, one short of / on / one past the 64-row tile; more tiles
    than the grid cap (512 workgroups below 72 KB of LDS, 256 above: workgroups loop); sq8_encode_wave 0 at a wave kernel's shape"""
    family = "tile" if n <= 65 else "tile_nowave" if n == 5000 else "tile_loop"
    run_family(amd, orc, family, d, n)


@gpu
@pytest.mark.parametrize("d,n", M.TWO_PASS + [M.TWO_PASS_LOOP])
def test_two_pass_kernels(amd, orc, d, n):
    """sq8_rownorm_kernel (64 rows per workgroup, 256 columns per step), sq8_train_kernel (512 rows), sq8_encode_kernel (16 rows,
    at most 4096 workgroups: the last case loops) at widths the single-pass kernels do not take"""
    run_family(amd, orc, "two_pass", d, n)


@gpu
@pytest.mark.parametrize("which", MISALIGN)
@pytest.mark.parametrize("d,n", M.MISALIGNED)
def test_alignment_fallbacks(amd, orc, d, n, which):
    """x one float, codes one byte or vmin one float off their alignment, at widths and row counts the group / wave kernels take
    otherwise: the two-pass kernels answer, with the oracle's bits"""
    key = (d, n, None)
    off = (1 if which == "x" else 0, 1 if which == "codes" else 0, 1 if which == "vmin" else 0)
    assert M.TRAIN2 not in names(M.train_launches(d, n, 1, True, T())) and M.ENCODE2 not in names(M.encode_launches(d, n, 1, True, True, True, True, T()))
    if which == "x":
        check_train(amd, orc, key, "misaligned", [T()], x_off=1)
    check_encode(amd, orc, key, "misaligned", [T()], off=off)
    _oracle_encode.cache_clear()


def check_decode(amd, orc, d, n, off=(0, 0, 0), expect_name=None):
    import torch
    vmin, vdiff, codes = M.decode_inputs(d, n)
    vm, vd, ct = dev(vmin, off[2]), dev(vdiff), dev(codes, off[1])
    for mode, entry, ref in ((0, "cvtmi_sq8_decode_dev", orc.sq8_decode), (1, "cvtmi_sq8_decode_faiss_dev", orc.sq8_decode_faiss)):
        out = dev_empty((n, d), torch.float32, off[0])
        out.fill_(float("nan"))
        with amd.launch_log() as log:
            rc = getattr(amd.lib(), entry)(ptr(vm), ptr(vd), C.c_int(d), ptr(ct), C.c_int64(n), ptr(out), stream())
        assert rc == 0
        expect = M.decode_launches(d, n, al(out, 16), al(ct, 4), al(vm, 16), al(vd, 16))
        assert log == expect, (d, n, mode, log, expect)
        assert expect_name is None or names(log) == [expect_name]
        got, exp = bits(out.cpu().numpy()), bits(ref(vmin, vdiff, codes))
        bad = np.argwhere(got != exp)
        assert bad.size == 0, (d, n, mode, bad[:4].tolist())


@gpu
@pytest.mark.parametrize("d,n", M.DECODE_TABLE)
def test_decode_table_kernel(amd, orc, d, n):
    """sq8_decode_lut_kernel from 16 384 rows (16 383: sq8_decode_kernel), both arithmetic modes: one column slab, a slab seam
    (124 / 132 / 260: the last slab 124, 4 and 4 columns wide), 16 slabs; row_splits cut by n / 2048 with a ragged last split,
    and (2048-d, 32 769 rows) the full 16 splits"""
    check_decode(amd, orc, d, n, expect_name=M.DEC_LUT if n >= 16_384 else M.DEC_VEC)


@gpu
@pytest.mark.parametrize("d,n,off", [(5, 100, (0, 0, 0)), (5, 16_385, (0, 0, 0)), (128, 16_385, (1, 0, 0)), (128, 16_385, (0, 1, 0)), (128, 16_383, (0, 0, 1))])
def test_decode_any_width_kernel(amd, orc, d, n, off):
    """sq8_decode_any_kernel, both modes: a width that is no multiple of 4, and d = 128 with the output rows one float, the codes one
    byte (above the table kernel's row count) or vmin one float (below it) off their alignment"""
    check_decode(amd, orc, d, n, off=off, expect_name=M.DEC_ANY)


@gpu
@pytest.mark.parametrize("d,n", HOST)
def test_host_entries(amd, orc, d, n):
    """the host-pointer entries stage into aligned buffers: the same routes, the same bits"""
    key = (d, n, None)
    x = table(*key)
    for l2 in (1, 0):
        with tuned(amd, T()), amd.launch_log() as log:
            vm, vd = amd.sq8_train(x.copy(), l2norm=l2)
        assert log == M.train_launches(d, n, l2, True, T()), (key, l2, log)
        ovm, ovd = oracle_train(orc, key, l2)
        assert np.array_equal(bits(vm), bits(ovm)) and np.array_equal(bits(vd), bits(ovd)), (key, l2)
    for l2 in (1, 2, 0):
        hv, hd = ranges(orc, key, l2)
        oc, ox = oracle_encode(orc, key, l2)
        fin, fin_cols = comparable(x, ox, hd)
        rows = x.copy()
        with tuned(amd, T()), amd.launch_log() as log:
            codes = amd.sq8_encode(hv, hd, rows, l2norm=l2)
        assert log == M.encode_launches(d, n, l2, True, True, True, True, T()), (key, l2, log)
        assert np.array_equal(codes[fin][:, fin_cols], oc[fin][:, fin_cols]), (key, l2)
        assert np.array_equal(bits(rows), bits(ox if l2 == 1 else x)), (key, l2)
    _oracle_encode.cache_clear()


@gpu
@pytest.mark.parametrize("d,n", [(132, 16_385), (5, 100), (128, 300)])
def test_host_decode_entries(amd, orc, d, n):
    vmin, vdiff, codes = M.decode_inputs(d, n)
    for fn, ref in ((amd.sq8_decode, orc.sq8_decode), (amd.sq8_decode_faiss, orc.sq8_decode_faiss)):
        with amd.launch_log() as log:
            out = fn(vmin, vdiff, codes)
        assert log == M.decode_launches(d, n, True, True, True, True), (d, n, log)
        assert np.array_equal(bits(out), bits(ref(vmin, vdiff, codes))), (d, n)
