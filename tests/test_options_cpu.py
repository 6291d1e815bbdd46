"""The options table (csrc/host_logic.cpp: kOptions, option_set, option_get, options_from_env) - what relax_set_option, relax_get_option and
relax_create's environment defaults go through - without a GPU: the key list, every rule's round trips, the refusals with their texts, and
the seven variables."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# key -> (default, rule).  Rules: "given" as given; "bool" != 0; ("floor", F) a non-positive value becomes F; ("one_of", a, b, text);
# ("range", lo, hi, text) - the last two refuse anything else with "relax_set_option: <key> must be <text>".
# A new option is one line here, one GemmOptions field and one row of kOptions.
OPTIONS = {
    "gemm_split_k": (1, "given"),
    "gemm_precision": (3, ("range", 0, 3, "0 (fp32), 1 (bf16x3), 2 (bf16x6) or 3 (f16x2)")),
    "gemm_variant": (-1, "given"),
    "gemm_variant_n64": (-1, "given"),
    "gemm_group_m": (8, ("floor", 1)),
    "flow_max_pairs": (0, ("floor", 0)),
    "flow_fused": (1, "bool"),
    "flow_seg_rows": (0, ("floor", 0)),
    "flow_pyramid_fused": (1, "bool"),
    "x6_fp32_rows": (1, "bool"),
    "rn_h2": (1, "bool"),
    "rn_h2_early": (1, "bool"),
    "rn_fuse": (1, "bool"),
    "rn_c1_h2": (1, "bool"),
    "b2b_rows": (256, ("one_of", 128, 256, "128 or 256")),
    "att_h2": (1, "bool"),
    "att_h2_stream": (1, "bool"),
    "h2_form": (1, ("range", 0, 2, "0, 1 or 2")),
    "h2_stages": (3, ("one_of", 3, 4, "3 or 4")),
    "debug_poison": (0, "bool"),
}
# variable -> key
ENV = {
    "RELAX_GEMM_SPLIT": "gemm_split_k",
    "RELAX_GEMM_PRECISION": "gemm_precision",
    "RELAX_H2_FORM": "h2_form",
    "RELAX_GEMM_VARIANT": "gemm_variant",
    "RELAX_GEMM_VARIANT_N64": "gemm_variant_n64",
    "RELAX_GEMM_GROUP_M": "gemm_group_m",
    "RELAX_DEBUG_POISON": "debug_poison",
}


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """csrc/host_logic.cpp alone with its test entry points, built into a temporary directory (plain g++, no HIP)."""
    out = tmp_path_factory.mktemp("host") / "libhost.so"
    src = os.path.join(ROOT, "relax-vqa_amd", "csrc", "host_logic.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DRELAX_HOST_TEST_API", src, "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.relax_host_option_key.restype = C.c_char_p
    lib.relax_host_options_new.restype = C.c_void_p
    lib.relax_host_options_free.argtypes = [C.c_void_p]
    lib.relax_host_option_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    lib.relax_host_option_get.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    lib.relax_host_options_from_env.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int]
    return lib


class Options:
    """a GemmOptions with its defaults; set / get return the value or the refusal's message"""

    def __init__(self, lib, env=None):
        self.lib, self.o = lib, lib.relax_host_options_new()
        if env is not None:
            n = len(env)
            names = (C.c_char_p * n)(*[k.encode() for k in env])
            values = (C.c_char_p * n)(*[v.encode() for v in env.values()])
            lib.relax_host_options_from_env(self.o, names, values, n)

    def close(self):
        self.lib.relax_host_options_free(self.o)

    def set(self, key, value):
        err = C.create_string_buffer(2048)
        rc = self.lib.relax_host_option_set(self.o, key if key is None else key.encode(), value, err, 2048)
        assert (rc == 0) == (err.value == b"") and rc in (0, -1)
        return None if rc == 0 else err.value.decode()

    def get(self, key, null_value=False):
        v, err = C.c_int(-12345), C.create_string_buffer(2048)
        rc = self.lib.relax_host_option_get(self.o, key if key is None else key.encode(), None if null_value else C.byref(v), err, 2048)
        assert (rc == 0) == (err.value == b"") and rc in (0, -1)
        return v.value if rc == 0 else err.value.decode()

    def all(self):
        return {k: self.get(k) for k in OPTIONS}


@pytest.fixture
def opts(host_lib):
    o = Options(host_lib)
    yield o
    o.close()


DEFAULTS = {k: d for k, (d, _) in OPTIONS.items()}


def test_the_table_has_exactly_these_keys_with_these_defaults(host_lib, opts):
    keys, i = [], 0
    while host_lib.relax_host_option_key(i) is not None:
        keys.append(host_lib.relax_host_option_key(i).decode())
        i += 1
    assert len(OPTIONS) == 20
    assert sorted(keys) == sorted(OPTIONS) and len(set(keys)) == len(keys)
    assert host_lib.relax_host_option_key(-1) is None
    assert opts.all() == DEFAULTS


def _accepted(rule):
    """(value set, value read back) pairs of a rule: every normalisation, both ends of a range, each member of a set"""
    if rule == "given":
        return [(-1, -1), (0, 0), (1, 1), (10, 10), (-2**31, -2**31), (2**31 - 1, 2**31 - 1)]
    if rule == "bool":
        return [(0, 0), (1, 1), (7, 1), (-1, 1), (0, 0)]
    if rule[0] == "floor":
        return [(5, 5), (0, rule[1]), (-3, rule[1]), (1, 1), (-1, rule[1]), (2**31 - 1, 2**31 - 1)]
    if rule[0] == "one_of":
        return [(rule[1], rule[1]), (rule[2], rule[2]), (rule[1], rule[1])]
    lo, hi = rule[1], rule[2]
    return [(v, v) for v in range(lo, hi + 1)] + [(lo, lo)]


def _refused(rule):
    if isinstance(rule, str) or rule[0] == "floor":
        return []
    if rule[0] == "one_of":
        a, b = rule[1], rule[2]
        return [v for v in (a - 1, b + 1, (a + b) // 2, 0, -a, a // 2, 2 * b) if v not in (a, b)]
    return [rule[1] - 1, rule[2] + 1, -2**31, 2**31 - 1]


@pytest.mark.parametrize("key", list(OPTIONS))
def test_round_trips_and_refusals(opts, key):
    default, rule = OPTIONS[key]
    others = {k: v for k, v in DEFAULTS.items() if k != key}
    for given, want in _accepted(rule):
        assert opts.set(key, given) is None, (key, given)
        assert opts.get(key) == want, (key, given)
        for bad in _refused(rule):      # a refused value leaves the stored one untouched
            assert opts.set(key, bad) == f"relax_set_option: {key} must be {rule[3]}", (key, bad)
            assert opts.get(key) == want, (key, bad)
        assert {k: v for k, v in opts.all().items() if k != key} == others   # ... and no key writes another's field


def test_the_examples_of_each_rule(opts):
    """the cases written out, against the literal texts"""
    for v in (0, -3):
        assert opts.set("gemm_group_m", v) is None and opts.get("gemm_group_m") == 1
    assert opts.set("flow_seg_rows", -1) is None and opts.get("flow_seg_rows") == 0
    assert opts.set("flow_max_pairs", -1) is None and opts.get("flow_max_pairs") == 0
    assert opts.set("rn_fuse", 7) is None and opts.get("rn_fuse") == 1
    for v in (-1, 10):
        assert opts.set("gemm_variant", v) is None and opts.get("gemm_variant") == v
    refusals = {
        "gemm_precision": ((-1, 4), "relax_set_option: gemm_precision must be 0 (fp32), 1 (bf16x3), 2 (bf16x6) or 3 (f16x2)"),
        "h2_form": ((-1, 3), "relax_set_option: h2_form must be 0, 1 or 2"),
        "h2_stages": ((2, 5), "relax_set_option: h2_stages must be 3 or 4"),
        "b2b_rows": ((64, 192), "relax_set_option: b2b_rows must be 128 or 256"),
    }
    for key, (values, text) in refusals.items():
        for v in values:
            assert opts.set(key, v) == text
            assert opts.get(key) == DEFAULTS[key]
    assert [k for k, (_, r) in OPTIONS.items() if not isinstance(r, str) and r[0] in ("one_of", "range")] == \
        ["gemm_precision", "b2b_rows", "h2_form", "h2_stages"]   # the four refusals are all there are


def test_unknown_empty_and_null_keys(opts):
    assert opts.set("no_such_option", 1) == "relax_set_option: unknown option 'no_such_option'"
    assert opts.get("no_such_option") == "relax_get_option: unknown option 'no_such_option'"
    assert opts.set("", 1) == "relax_set_option: unknown option ''"
    assert opts.get("") == "relax_get_option: unknown option ''"
    assert opts.set(None, 1) == "relax_set_option: key is NULL"
    assert opts.get(None) == "relax_get_option: NULL argument"
    assert opts.get("gemm_split_k", null_value=True) == "relax_get_option: NULL argument"
    for key in ("gemm_split_k ", "GEMM_SPLIT_K", "gemm_split", "gemm_split_kk", "profile_events", "workspace_mib"):   # (the two counters need the handle)
        assert opts.set(key, 0) == f"relax_set_option: unknown option '{key}'"
        assert opts.get(key) == f"relax_get_option: unknown option '{key}'"
    long_key = "k" * 1024
    assert opts.set(long_key, 1) == f"relax_set_option: unknown option '{long_key}'"
    assert opts.get(long_key) == f"relax_get_option: unknown option '{long_key}'"
    assert opts.all() == DEFAULTS


def _from_env(lib, env):
    o = Options(lib, env)
    got = o.all()
    o.close()
    return got


def test_environment_defaults(host_lib):
    assert _from_env(host_lib, {}) == DEFAULTS
    assert _from_env(host_lib, {"RELAX_NO_SUCH_VARIABLE": "5", "PATH": "0"}) == DEFAULTS
    assert len(ENV) == 7

    def one(var, text):
        got = _from_env(host_lib, {var: text})
        key = ENV[var]
        assert {k: v for k, v in got.items() if k != key} == {k: v for k, v in DEFAULTS.items() if k != key}, (var, text)
        return got[key]

    # each variable alone, with a value that differs from the default
    assert one("RELAX_GEMM_SPLIT", "0") == 0
    assert one("RELAX_GEMM_PRECISION", "2") == 2
    assert one("RELAX_H2_FORM", "2") == 2
    assert one("RELAX_GEMM_VARIANT", "7") == 7
    assert one("RELAX_GEMM_VARIANT_N64", "10") == 10
    assert one("RELAX_GEMM_GROUP_M", "4") == 4
    assert one("RELAX_DEBUG_POISON", "1") == 1
    # the rules, and the two fallbacks of a refused value
    assert [one("RELAX_GEMM_PRECISION", str(v)) for v in (0, 1, 2, 3)] == [0, 1, 2, 3]
    assert one("RELAX_GEMM_PRECISION", "9") == 0 and one("RELAX_GEMM_PRECISION", "-1") == 0
    assert [one("RELAX_H2_FORM", str(v)) for v in (0, 1, 2)] == [0, 1, 2]
    assert one("RELAX_H2_FORM", "9") == 1 and one("RELAX_H2_FORM", "-1") == 1
    assert one("RELAX_GEMM_GROUP_M", "0") == 1 and one("RELAX_GEMM_GROUP_M", "-8") == 1
    assert one("RELAX_DEBUG_POISON", "2") == 1 and one("RELAX_DEBUG_POISON", "0") == 0
    assert one("RELAX_GEMM_SPLIT", "5") == 5 and one("RELAX_GEMM_VARIANT", "-1") == -1
    # a value atoi cannot read is 0, then taken by the rule
    assert one("RELAX_GEMM_PRECISION", "f16x2") == 0 and one("RELAX_H2_FORM", "") == 0 and one("RELAX_GEMM_GROUP_M", "x") == 1
    assert one("RELAX_GEMM_SPLIT", "off") == 0 and one("RELAX_DEBUG_POISON", "yes") == 0
    # all seven at once
    got = _from_env(host_lib, {"RELAX_GEMM_SPLIT": "0", "RELAX_GEMM_PRECISION": "1", "RELAX_H2_FORM": "0", "RELAX_GEMM_VARIANT": "4",
                               "RELAX_GEMM_VARIANT_N64": "5", "RELAX_GEMM_GROUP_M": "16", "RELAX_DEBUG_POISON": "1"})
    assert got == {**DEFAULTS, "gemm_split_k": 0, "gemm_precision": 1, "h2_form": 0, "gemm_variant": 4, "gemm_variant_n64": 5, "gemm_group_m": 16,
                   "debug_poison": 1}
