"""CPU: every cvtmi_set_tuning key has the default and the rule written down here, read back through cvtmi_get_tuning.  The
table below is the record of what each key accepts, refuses and makes of its argument; csrc/tuning.def must agree with it
key by key (tests/test_abi.py checks that the two name the same keys)."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

EINVAL, EUNSUPPORTED = "EINVAL", "EUNSUPPORTED"
STATUS = {EINVAL: -1, EUNSUPPORTED: -5}   # CVTMI_EINVAL, CVTMI_EUNSUPPORTED
I32, I64 = 2 ** 31 - 1, 2 ** 63 - 1


# ---- the rules, as what they make of a value ----
def R(lo, hi):   # refused outside lo .. hi
    return ("R", lo, hi)


def C(lo, hi):   # moved to the nearer bound
    return ("C", lo, hi)


B = ("B", 0, 1)              # stores v != 0
A = ("C", -I32 - 1, I32)     # an int as given (beyond the int range: the nearer end of it)


def rule_result(rule, v):
    kind, lo, hi = rule
    if kind == "R":
        return v if lo <= v <= hi else EINVAL
    if kind == "C":
        return min(max(v, lo), hi)
    return int(v != 0)


def probes(rule):
    """both bounds, one past each, a negative value, 0, 1 and 2 -- what fits an int64"""
    _, lo, hi = rule
    vals = [lo, hi, lo - 1, hi + 1, -5, 0, 1, 2]
    return [(v, rule_result(rule, v)) for v in dict.fromkeys(vals) if -I64 - 1 <= v <= I64]


# the four keys whose rule is none of the above: every branch, spelled out
SPECIAL = {
    "scanh_fix": [(1, 1), (2, 2), (160000, 160000), (250000, 250000), (I64, I64), (0, 160000), (-1, 160000), (-5, 160000)],
    "scanh_min_rows": [(0, EINVAL), (-1, EINVAL), (-5, EINVAL), (1, 2048), (2, 2048), (2047, 2048), (2048, 2048), (2049, 2049),
                       (16384, 16384), (I64, I64)],
    "flat_u8_tfilter_chunks": [(-5, 1), (0, 1), (1, 1), (2, 2), (3, 2), (4, 4), (5, 4), (I32, 4), (I64, 4)],
    # a shipping build (no -DCVTMI_GF_DBG) refuses every value
    "flat_u8_dbg": [(v, EUNSUPPORTED) for v in (-5, 0, 1, 2, 3, I32)],
}

# (name, default, rule) in the order of csrc/tuning.def
TABLE = [
    ("assign_variant", 0, R(0, 2)),
    ("flat_variant", 0, R(0, 2)),
    ("probe_variant", 0, R(0, 2)),
    ("flat_f32_nt", 1, R(0, 2)),
    ("scanh_balance", 0, R(0, 2)),
    ("scans_dbg", 0, A),
    ("opq_host_chunk", 4096, R(0, 1 << 24)),
    ("scanh_fix", 160000, None),
    ("scanh_share_hist", 1, B),
    ("scanh_tail", 0, B),
    ("scanh_min_rows", 16384, None),
    ("scan_seed", 1, R(0, 1)),
    ("flat_f32_stream", 1, R(0, 2)),
    ("flat_f32_dbg", 0, A),
    ("flat_count_redo", 0, R(0, 1)),
    ("flat_f32_tfilter", 4, C(0, 4)),
    ("flat_f32_tfilter_min", 0, C(0, I32)),
    ("flat_f32_tfilter_one", 1 << 30, C(0, I32)),
    ("flat_f32_tfilter_bigk", 1, B),
    ("flat_f32_tfilter_retry", 0, B),
    ("flat_f32_tfilter_wide_band", 1, B),
    ("flat_f32_packed", 1, B),
    ("flat_f32_tfilter_min_rows", 262144, C(32768, I32)),
    ("flat_f32_tfilter_sample", 0, C(0, 64)),
    ("flat_f32_share", 0, R(0, 1)),
    ("flat_f32_rows_copy", 4, C(0, 1 << 20)),
    ("opq_small_zero_copy", 1, B),
    ("opq_host_zero_copy", 1, B),
    ("host_spin_us", 200, C(0, I32)),
    ("hnsw_top_lds", 256, C(0, I32)),
    ("hnsw_build_frac", 32, C(1, 1 << 30)),
    ("hnsw_build_cap", 8192, C(1, 1 << 30)),
    ("hnsw_build_phases", 0, B),
    ("hnsw_adc_tables", 0, B),
    ("hnsw_slots", 0, A),
    ("flat_u8_tfilter", 1, B),
    ("flat_u8_tfilter_min_rows", 262144, C(65536, I64)),
    ("flat_u8_tfilter_small_min_nq", 129, C(1, 1 << 30)),
    ("flat_u8_tfilter_min_k", 1, C(1, 1 << 20)),
    ("flat_u8_tfilter_min_nq", 129, C(1, 1 << 30)),
    ("flat_u8_tfilter_min_nq_k65", 97, C(1, 1 << 30)),
    ("flat_u8_tfilter_chunks", 4, None),
    ("flat_u8_tfilter_sample", 0, C(0, 64)),
    ("flat_u8_gfilter", 1, A),
    ("flat_u8_opt", 0, R(0, 3)),
    ("flat_u8_dbg", 0, None),
    ("flat_u8_mstream_min", 1, R(1, 129)),
    ("flat_u8_mstream_min_rows", 4096, C(4096, I64)),
    ("flat_u8_filter_min_nq", 129, C(1, 1 << 30)),
    ("flat_u8_filter_min_rows", 524288, C(0, I64)),
    ("flat_u8_filter_min_work", 130, C(0, I64)),
    ("flat_u8_sample_passes", 10, C(0, 64)),
    ("flat_small_zero_copy", 1, B),
    ("sq8_encode_wave", 1, B),
    ("sq8_filter", 1, B),
    ("sq8_flags", 1, A),
    ("sq8_wave_blocks", 3, R(1, 64)),
    ("sq8_host_small", 1, B),
    ("scan_pad_m", 1, B),
    ("scan_packed_m", 1, B),
    ("scan_bigk", 1, B),
    ("scans_max_work", 48 << 20, C(0, I64)),
    ("scan_tail_splits", 0, A),
    ("ivf_part_cap_mb", 256, R(0, 4096)),
    ("ivf_range_spill", 4096, R(0, I64)),
    ("comm_force_rccl", 0, B),
    ("comm_check_status", 2, B),   # (so its default cannot be set back: 2 stores 1)
    ("comm_inject_failure", -1, A),
]
KEYS = [name for name, _, _ in TABLE]


def expected_probes(name, rule):
    return SPECIAL[name] if rule is None else probes(rule)


def _lib():
    import cvt_amd
    lib = cvt_amd.lib()
    lib.cvtmi_last_error.restype = ctypes.c_char_p
    return lib


def _get(lib, name):
    v = ctypes.c_int64(-12345)
    assert lib.cvtmi_get_tuning(name.encode(), ctypes.byref(v)) == 0, name
    return v.value


def sweep(lib, rows):
    """every probe of every row: what a set returns, what a get reads back afterwards"""
    for name, _, rule in rows:
        for value, want in expected_probes(name, rule):
            before = _get(lib, name)
            rc = lib.cvtmi_set_tuning(name.encode(), ctypes.c_int64(value))
            if want in STATUS:   # refused: the status, a message that names the key, the stored value untouched
                assert rc == STATUS[want], (name, value, rc)
                assert name.encode() in lib.cvtmi_last_error(), (name, value)
                assert _get(lib, name) == before, (name, value)
            else:
                assert rc == 0, (name, value, lib.cvtmi_last_error())
                assert _get(lib, name) == want, (name, value)


def _child(args, spin_env=None):
    """this file as a program in a fresh process: the library loaded, nothing set"""
    from cvt_amd import capi
    env = {k: v for k, v in os.environ.items() if k != "CVTMI_HOST_SPIN_US"}
    if spin_env is not None:
        env["CVTMI_HOST_SPIN_US"] = spin_env
    return subprocess.run([sys.executable, os.path.abspath(__file__), capi.LIB_PATH] + args, env=env, capture_output=True, text=True, check=True).stdout


def test_table_is_well_formed():
    assert len(KEYS) == len(set(KEYS)) == 68
    assert sorted(SPECIAL) == sorted(name for name, _, rule in TABLE if rule is None)
    for name, default, rule in TABLE:
        assert {-5, 0, 1, 2} <= {v for v, _ in expected_probes(name, rule)}, name
        if rule is not None and rule[0] != "B":   # the default is a value the rule stores as it is
            assert rule_result(rule, default) == default, name


@pytest.mark.parametrize("spin_env", [None, "7"])
def test_defaults_of_a_fresh_process(spin_env):
    got = json.loads(_child(["defaults"], spin_env))
    want = {name: default for name, default, _ in TABLE}
    if spin_env is not None:
        want["host_spin_us"] = int(spin_env)
    assert got == want


# "comm_check_status" stores v != 0 although its default is 2: no set brings the default back.  Its probes run in a process of
# their own, so that the tests after this one still run under the default.
NO_WAY_BACK = "comm_check_status"


def test_every_rule_through_set_and_get():
    lib = _lib()
    rows = [r for r in TABLE if r[0] != NO_WAY_BACK]
    spin = max(0, int(os.environ.get("CVTMI_HOST_SPIN_US", "200")))   # this process's default of "host_spin_us"

    def restore():
        for name, default, _ in rows:
            if name != "flat_u8_dbg":   # (never left its default: every set is refused)
                assert lib.cvtmi_set_tuning(name.encode(), ctypes.c_int64(spin if name == "host_spin_us" else default)) == 0, name

    try:
        sweep(lib, rows)
    finally:
        restore()
    for name, default, _ in rows:
        assert _get(lib, name) == (spin if name == "host_spin_us" else default), name


def test_rule_of_the_key_without_a_way_back():
    assert _child(["sweep", NO_WAY_BACK]).strip() == "swept 1"
    assert _get(_lib(), NO_WAY_BACK) == 2


def test_get_tuning_validates_its_arguments():
    lib = _lib()
    v = ctypes.c_int64(77)
    assert lib.cvtmi_get_tuning(None, ctypes.byref(v)) == -1
    assert lib.cvtmi_get_tuning(b"flat_variant", None) == -1
    assert lib.cvtmi_get_tuning(b"no_such_knob", ctypes.byref(v)) == -1 and b"no_such_knob" in lib.cvtmi_last_error()
    assert v.value == 77
    import cvt_amd
    assert cvt_amd.get_tuning("sq8_wave_blocks") == 3
    with pytest.raises(cvt_amd.CvtmiError):
        cvt_amd.get_tuning("no_such_knob")


if __name__ == "__main__":   # the child of _child(): argv = library, "defaults" | "sweep" key ...
    child_lib = ctypes.CDLL(sys.argv[1])
    child_lib.cvtmi_last_error.restype = ctypes.c_char_p
    if sys.argv[2] == "defaults":
        print(json.dumps({name: _get(child_lib, name) for name in KEYS}))
    else:
        picked = [r for r in TABLE if r[0] in sys.argv[3:]]
        sweep(child_lib, picked)
        print("swept %d" % len(picked))
