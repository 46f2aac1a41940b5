"""The single-chain columns of field30.hip.h on the device.

Products: fq_mul, fq_sqr, fq_mul_sub, fq_mul_minus, fq_mul_plus and fq_sqr_minus as hipcc compiles them with the switch of
msm_accum.hip (tests/device_columns/columns.hip: KZG_F30_SERIAL_COLUMNS, one wave per row, every lane writes its result)
against the g++ build of the same header (tests/host/field30_columns_host.cpp), digit for digit, on that file's rows: the
edges of the contracts (every digit at +-2^29 and +-(2^29 + 4), one multiplicand a raw sum of two, values taken into the
carry pass at +-(2^31 - 1), 0, +-p, +-3p) and random rows.  tests/test_field30_columns.py shows on the CPU that the g++
build returns the digits of the earlier definitions.

Kernel: k_bucket_accumulate itself at 4369 and 8193 terms -- jobs of more than 65536 references, so the general kernels and
not k_small_msm -- on the bench polynomial c_i = 5^i + 10 and on all-equal coefficients, with the bench setup and with the
setups s = 0, 1, -1, where the lanes meet infinity, doubling and cancellation.  48-byte commitments against [P(s)]G
(tests/trapdoor_oracle.py)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import bigint_twin as T
import kzg_poly_commit_exploration_amd as K
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "device_columns", "libkzg_devcolumns.so")
HOST_SRC = os.path.join(ROOT, "tests", "host", "field30_columns_host.cpp")
OPS = ["fq_mul", "fq_sqr", "fq_mul_sub", "fq_mul_minus", "fq_mul_plus", "fq_sqr_minus"]
RANDOM_ROWS = 768  # behind the edge rows: 1024 waves per function
R = TO.R
GOLDEN_S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("f30c") / "libf30c.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", out, HOST_SRC], check=True)
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def device():
    if not os.path.exists(HARNESS):
        if shutil.which("hipcc") is None:
            raise RuntimeError("%s is missing and there is no hipcc to build it with: run __graft_entry__.build() (or make -C "
                               "tests/device_columns) where ROCm is installed" % HARNESS)
        subprocess.run(["make", "-s", "-C", os.path.dirname(HARNESS)], check=True)
    return ctypes.CDLL(HARNESS)


def i32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


@pytest.mark.parametrize("op", range(len(OPS)), ids=OPS)
def test_products_on_the_device_match_the_host_digit_for_digit(host, device, op):
    assert host.f30c_ops() == len(OPS)
    n = host.f30c_edge_rows() + RANDOM_ROWS
    rows = np.zeros((n, 52), dtype=np.int32)
    host.f30c_rows(op, 0, n, i32p(rows))
    want = np.zeros((n, 13), dtype=np.int32)
    host.f30c_run(op, i32p(rows), n, i32p(want))
    got = np.zeros((n, 64, 13), dtype=np.int32)
    status = device.devcol_run(op, i32p(rows), n, i32p(got))
    assert status == 0, "HIP status %d" % status
    bad = np.argwhere((got != want[:, None, :]).any(axis=2))
    assert bad.size == 0, "%s: %d (row, lane) pairs differ from the host; first: row %d lane %d, device %s, host %s" % (
        OPS[op], len(bad), bad[0][0], bad[0][1], got[bad[0][0], bad[0][1]].tolist(), want[bad[0][0]].tolist())


def limbs_of(vals):
    """Montgomery limbs; repeated values are converted once"""
    distinct = {}
    idx = np.fromiter((distinct.setdefault(v % R, len(distinct)) for v in vals), dtype=np.int64, count=len(vals))
    return np.ascontiguousarray(K.scalars_to_limbs(list(distinct))[idx])


def coefficient_vectors(n):
    bench, c = [], 1
    for _ in range(n):
        bench.append((c + 10) % R)
        c = c * 5 % R
    return [("bench polynomial 5^i + 10", bench), ("all equal", [bench[n // 2]] * n)]


@pytest.mark.parametrize("n", [4369, 8193])
@pytest.mark.parametrize("secret", [GOLDEN_S, 0, 1, R - 1], ids=["s=bench", "s=0", "s=1", "s=-1"])
def test_accumulation_kernel_commitments(oracle, secret, n):
    job = TO.Job(n, n)
    assert not job.small and job.max_refs > TO.K_TINY_REFS  # the general kernels: k_bucket_accumulate
    eng = K.SetupArtifactsGenerator(TO.secret_be(secret)).take(n)
    try:
        for label, vals in coefficient_vectors(n):
            assert eng.commit_limbs(limbs_of(vals)).compress() == TO.commitment(oracle, vals, secret), label
    finally:
        eng.close()
