"""The comparison rule of tests/test_gpu_dense_prologue.py on numpy arrays alone (no GPU): it rejects the ways a rotation, table or
projection kernel goes subtly wrong, reports the first differing row, its 32-row slab and its column, and accepts NaNs of different
payload where arithmetic made them."""
import numpy as np
import pytest

from conftest import bits
from test_gpu_dense_prologue import assert_same, assert_within_1ulp, first_mismatch

F32 = np.float32


def reference():
    rng = np.random.default_rng(3)
    ref = rng.normal(size=(96, 40)).astype(F32)
    ref[5, 7] = 0.0
    ref[40, 2] = np.inf
    ref[70, 9] = np.nan
    ref[71, 0] = -0.0
    ref[72, 1] = F32(1e-41)   # subnormal
    return ref


def test_equal_arrays_pass():
    ref = reference()
    assert first_mismatch(ref.copy(), ref) is None
    assert first_mismatch(ref.copy(), ref, nan_payload=True) is None
    assert first_mismatch(np.zeros((0, 8), F32), np.zeros((0, 8), F32)) is None
    assert_same(ref.copy(), ref, "copy")


def test_two_slabs_exchanged():
    ref = reference()
    got = ref.copy()
    got[32:64], got[64:96] = ref[64:96], ref[32:64]
    assert first_mismatch(got, ref) == (32, 1, 0)
    with pytest.raises(AssertionError, match=r"row 32 \(slab 1\) column 0"):
        assert_same(got, ref, "exchanged")


def test_one_stale_row():
    ref = reference()
    got = ref.copy()
    got[77] = 0
    assert first_mismatch(got, ref) == (77, 2, 0)


def test_one_ulp():
    ref = reference()
    got = ref.copy()
    got[33, 21] = np.nextafter(ref[33, 21], F32(np.inf))
    assert first_mismatch(got, ref) == (33, 1, 21)
    got = ref.copy()
    got[72, 1] = np.nextafter(ref[72, 1], F32(0))    # among subnormals too
    assert first_mismatch(got, ref) == (72, 2, 1)


def test_signed_zero():
    ref = reference()
    got = ref.copy()
    got[5, 7] = -0.0
    assert got[5, 7] == ref[5, 7] and first_mismatch(got, ref) == (5, 0, 7)
    got = ref.copy()
    got[71, 0] = 0.0
    assert first_mismatch(got, ref) == (71, 2, 0)


def test_nan_for_infinity_and_number_for_nan():
    ref = reference()
    got = ref.copy()
    got[40, 2] = np.nan
    assert first_mismatch(got, ref) == (40, 1, 2)
    got = ref.copy()
    got[70, 9] = 1.0
    assert first_mismatch(got, ref) == (70, 2, 9)
    got = ref.copy()
    got[40, 2] = -np.inf
    assert first_mismatch(got, ref) == (40, 1, 2)


def test_nan_payloads():
    ref = reference()
    got = ref.copy()
    got.view(np.uint32)[70, 9] = 0xFFC12345     # another sign and payload
    assert np.isnan(got[70, 9]) and bits(got)[70, 9] != bits(ref)[70, 9]
    assert first_mismatch(got, ref) is None                             # arithmetic: any NaN for a NaN
    assert first_mismatch(got, ref, nan_payload=True) == (70, 2, 9)     # the gather: bits


def test_tables_are_rows_of_their_first_dimension():
    ref = np.arange(3 * 4 * 5, dtype=F32).reshape(3, 4, 5)
    got = ref.copy()
    got[2, 1, 3] += 1
    assert first_mismatch(got, ref) == (2, 0, 8)


def test_one_ulp_rule_of_the_normalised_projection():
    ref = reference()
    got = ref.copy()
    got[33, 21] = np.nextafter(ref[33, 21], F32(np.inf))
    got.view(np.uint32)[70, 9] = 0xFFC12345
    assert_within_1ulp(got, ref, "one ulp, another NaN")
    got[33, 21] = np.nextafter(got[33, 21], F32(np.inf))
    with pytest.raises(AssertionError, match=r"row 33 \(slab 1\) column 21"):
        assert_within_1ulp(got, ref, "two ulps")
    got = ref.copy()
    got[40, 2] = np.nan
    with pytest.raises(AssertionError, match="row 40"):
        assert_within_1ulp(got, ref, "NaN for +inf")
    got = ref.copy()
    got[70, 9] = 0.0
    with pytest.raises(AssertionError, match="row 70"):
        assert_within_1ulp(got, ref, "a number for NaN")
