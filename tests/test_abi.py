"""Header and code in step (CPU only)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tuning_keys():
    """the keys of cvtmi_set_tuning / cvtmi_get_tuning: the names of csrc/tuning.def, in its order"""
    text = open(os.path.join(ROOT, "cvt_amd", "csrc", "tuning.def")).read()
    return re.findall(r"^TUNE\(([a-z0-9_]+),", text, flags=re.M)


def test_every_tuning_key_is_documented():
    """cvtmi_set_tuning's keys (csrc/tuning.def) and their description in include/cvtmi.h stay in step: a key the header does not name is a
    switch nobody can find."""
    hdr = open(os.path.join(ROOT, "include", "cvtmi.h")).read()
    keys = tuning_keys()
    assert len(keys) == 68
    missing = [k for k in keys if '"%s"' % k not in hdr]
    assert not missing, missing


def test_tuning_list_and_expected_table_name_the_same_keys():
    """tests/test_tuning_table.py holds the default and the rule of every key: a key added to the list is added there"""
    import test_tuning_table
    assert tuning_keys() == test_tuning_table.KEYS


def test_tuning_keys_live_in_the_list_only():
    """no key is compared by name in api.hip any more: cvtmi_set_tuning walks the objects the list generates"""
    api = open(os.path.join(ROOT, "cvt_amd", "csrc", "api.hip")).read()
    assert 'strcmp(name, "' not in api
