"""The field and group-law primitives as hipcc compiles them for the device, against Python integers.

tests/device/prims.hip wraps every primitive of field30.hip.h, field30_inv.hip.h, fr30.hip.h and g1_30.hip.h in one small
kernel (libkzg_devprims.so, built by __graft_entry__.build(); not part of the library).  Every table of
tests/prim_cases.py goes through it with one launch, and every case must satisfy the table's check: the value against the
integers, the digit ranges and magnitudes the headers state, exact zeros for infinity, identical digits in the four lanes of
a quad.  The quad tables place chosen case kinds in chosen quads of a wave (uniform waves, one or two live quads among
idle ones, alternating and random mixtures), call xyzz30_add_quad from every quad and from behind a branch on the quad, and
xyzz30_add_quad_dense straight and inside a loop whose trip count differs per quad.

The accumulation kernel's arithmetic has two families of its own.  accum_fused_products: fq_mul_minus, fq_mul_plus and
fq_sqr_minus must return exactly the product's integer (mont_py) minus or plus the third value, in strictly balanced digits,
with that value anything up to a raw sum of four (every digit at +-(2^31 - 4)); here the +-1 factor of the device form (kept
opaque in a scalar register, one v_mad_i64_i32) is what runs, which no g++ build compiles.  fq_maybe_zero is true on every
digit form of k p, |k| <= 3, and -- by design -- on other values that share digit 0 with one.  accum_mixed_addition:
xyzz30_acc_head, _rare and _tail against the integers of the same formulas digit for digit; xyzz30_acc_madd on the six case
kinds plus constructed false positives of the pre-test (P = t + k p with t = 0 mod 2^30, never equal or opposite), half of
the accumulators with X as the kernel holds it (a raw sum of two, digits up to 2^30), unsettled and settled; chains with a
false positive built against the known digits of step 6; and k_acc_dispatch, a device-only kernel that copies the shape of
k_bucket_accumulate around accum_rare_call (the wave-uniform ballot branch, the second read of a run's first point, the call
through a struct in private memory that hands acc, P and Rn back, the tail last): 35 whole waves of chosen lane kinds --
uniform, one rare lane among general ones, every kind at once, random mixtures -- in which every lane must return what the
single-lane addition returns.

A failure names the table, the case and its kind, for quad tables the wave composition and the quad, and says whether the
g++ build of the same function satisfies the same check on that case: if it does, the source is right and the device code
is not.

What this checks and what it does not: the headers as hipcc compiles them for gfx950 inside a small kernel.  The library's
kernels inline the same functions in other surroundings (other register pressure, other neighbours for the scheduler), so
the end-to-end tests remain the check of those kernels."""
import ctypes
import os
import shutil
import subprocess

import pytest

import prim_cases as C
from test_device_prims import build_host_libs, make_runner, run_table

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "device", "libkzg_devprims.so")


@pytest.fixture(scope="module")
def device_run():
    if not os.path.exists(HARNESS):
        if shutil.which("hipcc") is None:
            raise RuntimeError("%s is missing and there is no hipcc to build it with: run __graft_entry__.build() (or make -C "
                               "tests/device) where ROCm is installed" % HARNESS)
        subprocess.run(["make", "-s", "-C", os.path.dirname(HARNESS)], check=True)
    lib = ctypes.CDLL(HARNESS)
    return make_runner(lambda op: lib, "devprim_")


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    return make_runner(build_host_libs(str(tmp_path_factory.mktemp("prims_host"))), "prim_")


def _report(table, bad, host_out):
    lines = ["%s: %d of %d cases fail on the device" % (table.name, len(bad), table.n)]
    for i, msg in bad[:5]:
        if host_out is None:
            host = "no host form of this primitive"
        else:
            host_msg = table.check(table.rows[i], table.wants[i], [int(v) for v in host_out[i]])
            host = "the host build agrees with Python here" if host_msg is None else "the host build fails too: " + host_msg
        lines.append("  case %d, kind %s%s: %s [%s]" % (i, table.kinds[i], ", " + table.where[i] if table.where[i] else "", msg, host))
    return "\n".join(lines)


@pytest.mark.parametrize("name", sorted(C.FAMILIES))
def test_primitives_on_the_device(device_run, host_run, name):
    reports = []
    for table in C.family(name):
        out = run_table(device_run, table, False)  # one launch
        bad = C.failures(table, out)
        if bad:
            reports.append(_report(table, bad, None if table.host is False else run_table(host_run, table, True)))
    assert not reports, "\n".join(reports)
