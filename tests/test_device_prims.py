"""The case tables of tests/prim_cases.py through the HOST build of the csrc headers (g++; tests/host/field30_host.cpp and
fr30_host.cpp export every primitive in the record form of tests/device/prim_ops.h).  This proves the tables and their
big-integer expectations before a GPU sees them: tests/test_device_prims_gpu.py asserts the same things of the device
build.  The quad primitives exist on the device only; their tables go through xyzz30_add here, with the same
expectations.  CPU only."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import prim_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32P = ctypes.POINTER(ctypes.c_int32)


def _ptr(a):
    return a.ctypes.data_as(I32P)


def make_runner(lib_of, prefix):
    """run(op, records, ints per result) -> results, through the export prefix + op of the library lib_of(op)"""
    def run(op, rows, ow, batches=None):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        n, iw = rows.shape
        out = np.empty((n, ow), dtype=np.int32)
        fn = getattr(lib_of(op), prefix + op)
        if batches is None:
            rc = fn(_ptr(rows), iw, _ptr(out), ow, n)
        else:
            off = np.array(batches, dtype=np.int32)
            rc = fn(_ptr(rows), iw, _ptr(off), len(batches) - 1, _ptr(out), ow, n)
        assert rc == 0, "%s%s returned %d" % (prefix, op, rc)
        return out
    return run


def run_table(run, table, host):
    """the output records of one table; host: through the g++ build (device-only primitives by their host stand-in)"""
    if host and table.host:
        return table.host(run, table)
    return run(table.op, table.inputs(), table.ow, table.batches)


def build_host_libs(tmp):
    libs = {}
    for name in ("field30", "fr30"):
        out = os.path.join(tmp, "lib%s_prims.so" % name)
        subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "host", name + "_host.cpp")], check=True)
        libs[name] = ctypes.CDLL(out)
    return lambda op: libs["fr30" if op in C.FR_OPS else "field30"]


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    return make_runner(build_host_libs(str(tmp_path_factory.mktemp("prims"))), "prim_")


@pytest.mark.parametrize("name", sorted(C.FAMILIES))
def test_tables_on_the_host_build(host_run, name):
    for table in C.family(name):
        assert 0 < table.n <= 4096
        if table.host is False:  # the quad moves: no host form; the expectations are restated digits
            continue
        bad = C.failures(table, run_table(host_run, table, True))
        assert not bad, "%s: %d of %d cases fail; first: case %d (%s) %s: %s" % (
            table.name, len(bad), table.n, bad[0][0], table.kinds[bad[0][0]], table.where[bad[0][0]], bad[0][1])


def test_tables_hold_what_they_promise():
    """the kinds and compositions that the tables exist for are all there"""
    madd, add = C.family("group_law_one_lane")[:2]
    for t in (madd, add):
        for kind in C.KINDS:
            for variant in ("extreme", "random"):
                assert sum(1 for k in t.kinds if k.startswith(kind) and k.endswith(variant)) >= 32, (t.name, kind, variant)
    waves = C.wave_compositions()
    names = [n for n, _ in waves]
    assert all(len(k) == 16 for _, k in waves)
    assert sum(n.startswith("uniform") for n in names) == 6 and sum(n.startswith("random mixture") for n in names) == 32
    assert sum(n.startswith("lone") for n in names) == 18 and sum(n.startswith("two live") for n in names) == 6
    assert sum(n.startswith("alternating") for n in names) == 4
    for t in C.family("quad_sparse") + C.family("quad_dense"):
        assert t.n == 16 * len(waves)
    sizes = np.diff(C.family("affine_pairs")[1].batches).tolist()
    assert sorted(set(sizes)) == [1, 2, 7, 64]
    pairs = C.family("affine_pairs")[1]
    assert any(all(w[0] not in (1, 2) for w in pairs.wants[a:b]) for a, b in zip(pairs.batches, pairs.batches[1:]))
    assert {w[0] for w in pairs.wants} == {1, 2, 3, 4, 5}
    assert {w[0] for w in C.family("affine_pairs")[0].wants} == {1, 2, 3, 4, 5}
    trips = {k.split("trip=")[1] for k in C.family("quad_dense")[1].kinds}
    assert trips == {"0", "1", "2", "3"}


def test_zero_tests_of_the_mixed_addition_reach_3p():
    """P = U2 - X1 of xyzz30_madd is a multiple k p when the operands are equal or opposite; with X1 up to 2.6 p the table
    must contain k = +-3 (the last multiple fq_is_zero knows), or a zero test cut down to |k| <= 2 would go unnoticed.
    R = S2 - Y1 stays below 2 p, so |k| <= 1 there."""
    seen = C.madd_zero_multiples(C.family("group_law_one_lane")[0])
    assert -3 in seen["P"] and 3 in seen["P"], sorted(seen["P"])
    assert max(abs(k) for k in seen["P"]) == 3
    assert set(seen["R"]) <= {-1, 0, 1} and {-1, 1} <= set(seen["R"]), sorted(seen["R"])


def test_accumulation_tables_hold_what_they_promise():
    """the tables of the accumulation kernel's addition: every kind x neg x representative x digit form of X, the zero tests at
    every multiple of p the magnitude line allows (|P| < 3.3 p: k = -3 .. 3; |R| < 2 p: k = -1 .. 1), false positives
    everywhere, and the wave compositions of the dispatch kernel"""
    head, rare, tail, madd, chain, dispatch = C.family("accum_mixed_addition")
    for kind in C.ACC_KINDS:
        for neg in (0, 1):
            for variant in ("extreme", "random"):
                for form in ("raw", "balanced"):
                    label = "%s neg=%d %s X %s" % (kind, neg, variant, form)
                    assert sum(1 for k in madd.kinds if k == label) >= 12, label
    assert head.rows == madd.rows
    for t in (madd, dispatch):
        seen = C.acc_zero_multiples(t)
        assert set(seen["P"]) == set(range(-3, 4)), (t.name, sorted(seen["P"]))
        assert set(seen["R"]) == {-1, 0, 1}, (t.name, sorted(seen["R"]))
        assert seen["false_positive"] >= 96
    assert sum(1 for k in madd.kinds if "every digit" in k) == 12  # X at the ends of the raw sum's range
    assert {w[0] for w in head.wants} == {0, 1, 4, 6, 7}             # (a fresh lane's P is exactly zero: it carries 4 as well)
    flags = [(k.split()[0], w[0], w[1] is None) for k, w in zip(rare.kinds, rare.wants)]
    assert {f for f in flags} == {("false_positive", 1, True), ("equal", 0, False), ("opposite", 0, True)}
    assert sum(f[0] == "false_positive" for f in flags) >= 96 and tail.n >= 192
    assert chain.n == 64 and C.FP_STEP == 7
    waves = C.dispatch_waves()
    names = [n for n, _ in waves]
    assert all(len(k) == 64 for _, k in waves) and dispatch.n == 64 * len(waves)
    assert sum(n.startswith("uniform") for n in names) == 7 and sum(n.startswith("lone") for n in names) == 18
    assert sum(n.startswith("every kind") for n in names) == 2 and sum(n.startswith("random mixture") for n in names) == 8
    assert all(set(k) == set(C.LANE_KINDS) for n, k in waves if n.startswith("every kind"))
    c_forms = {k.split(" c=")[1] for k in C.family("accum_fused_products")[0].kinds}
    assert {"0", "raw sum of 1", "raw sum of 4", "+1 (2^31-4), digit 12 -1 2^24", "-1 (2^31-4), digit 12 +1 2^24", "-2^31"} <= c_forms
    zero = C.family("accum_fused_products")[3]
    for k in range(-3, 4):
        for form in ("canonical", "re-split at digit 0", "raw difference", "norm(raw difference)"):
            assert any(kd == "%dp %s" % (k, form) and w == 1 for kd, w in zip(zero.kinds, zero.wants)), (k, form)
        assert sum(kd == "near miss of %dp" % k for kd in zero.kinds) == 16
    assert sum(w == 0 for w in zero.wants) >= 512


def test_mont_py_is_the_multiplier(host_run):
    """mont_py (used above to name the multiples) returns the very integer fq_mul returns"""
    t = C.family("fp_products")[0]
    out = run_table(host_run, t, True)
    for i in range(0, t.n, 7):
        assert C.value([int(v) for v in out[i]]) == C.mont_py(C.value(t.rows[i][:13]), C.value(t.rows[i][13:]))


def _hipflags(path):
    with open(path) as f:
        lines = [line for line in f if re.match(r"HIPFLAGS\s*\?=", line)]
    assert len(lines) == 1, path
    return lines[0]


def test_harness_is_built_with_the_flags_of_the_library():
    assert _hipflags(os.path.join(ROOT, "tests", "device", "Makefile")) == \
        _hipflags(os.path.join(ROOT, "kzg_poly_commit_exploration_amd", "csrc", "Makefile"))
