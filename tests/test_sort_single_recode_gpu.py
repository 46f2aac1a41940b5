"""The general MSM sort with ONE conversion per scalar: k_sort_count folds every scalar and leaves |k| and the negate flag in a
32-byte record, the spread pass cuts its digits from that record (msm_sort.hip, msm_recode.h).  Every case is checked against
the trapdoor oracle [P(s)]G (tests/trapdoor_oracle.py).

Shapes: the smallest that reach the multi-launch sort (n > 4096: not k_sort_small) and the accumulation kernel (more than
65536 references: not k_small_msm) -- 4369 terms (18 tiles of 256 scalars, the last one of 17), 4369 + 255 and 8193 (the last
tile partial / of one scalar; a tile is half a stride of the 512-lane workgroups), 65537, and a batch of two polynomials whose
stride is not their length.  Tiles of several strides with a partial last stride are what tests/test_msm_boundaries_gpu.py
runs at 2^20 + 1 terms (tile 2304 = 4.5 strides).  Both input forms, Montgomery images and canonical bytes.
Scalars: the edges of the fold and of the windows (tests/test_msm_recode_host.py) spread over the polynomial, all coefficients
equal (every reference of a window in one bucket), coefficients below 2^12 (the upper windows are zero digits), uniform ones.
The widths the kernels are compiled for (15, 16, 17, 19), one that takes the run-time loop (13), NAF, the direct spread and
two-word pairs run in one fresh process each: the engine reads those switches when it is created."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import bigint_twin as T
import kzg_poly_commit_exploration_amd as K
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu

R = TO.R
BENCH_S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)
HERE = os.path.dirname(os.path.abspath(__file__))
N_MIN = 4369  # one past 65536 / 15 terms
SHAPES = [N_MIN, N_MIN + 255, 8193, 65537]
WIDTHS = range(8, 21)


def every_window(c, w):
    return sum(w << (c * j) for j in range((255 + c - 1) // c)) & ((1 << 254) - 1)


def edge_scalars():
    s = [0, 1, R - 1, (R - 1) // 2, (R + 1) // 2, ((1 << 254) - 1) % R]
    for c in WIDTHS:
        s += [every_window(c, 1 << (c - 1)) % R, every_window(c, (1 << (c - 1)) + 1) % R]
    return s


def scalar_sets(n):
    """(label, values) of the four families at n terms"""
    rng = random.Random(n)
    edges = edge_scalars()
    spread = [edges[i % len(edges)] for i in range(n)]
    rng.shuffle(spread)
    equal = rng.randrange(R)
    return [("edges", spread), ("equal", [equal] * n), ("below 2^12", [rng.randrange(1 << 12) for _ in range(n)]),
            ("uniform", [rng.randrange(R) for _ in range(n)])]


def montgomery(vals):
    distinct = {}
    idx = np.fromiter((distinct.setdefault(v % R, len(distinct)) for v in vals), dtype=np.int64, count=len(vals))
    return np.ascontiguousarray(K.scalars_to_limbs(list(distinct))[idx])


def canonical(vals):
    return b"".join((v % R).to_bytes(32, "little") for v in vals)


_cases = {}


def cases(oracle, n):
    """(label, values, expected compressed commitment) per family, computed once per length"""
    if n not in _cases:
        _cases[n] = [(label, vals, TO.commitment(oracle, vals, BENCH_S)) for label, vals in scalar_sets(n)]
    return _cases[n]


def check_all(oracle, eng, n, mont, where=""):
    for label, vals, want in cases(oracle, n):
        got = eng.commit_limbs(montgomery(vals)) if mont else eng.commit_le_bytes(canonical(vals))
        assert got.compress() == want, "%s%s, n=%d, %s" % (where, label, n, "Montgomery" if mont else "canonical")


@pytest.mark.parametrize("mont", [True, False], ids=["montgomery", "canonical"])
@pytest.mark.parametrize("n", SHAPES)
def test_general_sort_at_its_smallest_shapes(engines, oracle, n, mont):
    eng = engines.bench_srs(n)
    cfg = eng.msm_config()
    assert n > 4096 and n * cfg["table_levels"] > 65536  # the multi-launch sort and the accumulation kernel
    check_all(oracle, eng, n, mont)


def test_batch_of_two_with_a_stride_that_is_not_the_length(engines, oracle):
    n, stride = N_MIN, N_MIN + 37
    eng = engines.bench_srs(n)
    sets = cases(oracle, n)
    before = eng.max_batch()
    try:
        assert eng.set_max_batch(2) == 2
        for a, b in ((0, 3), (1, 2)):  # edges + uniform, equal + small
            flat = np.full((2 * stride, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)  # the gap is not a scalar below r
            flat[:n] = montgomery(sets[a][1])
            flat[stride:stride + n] = montgomery(sets[b][1])
            dptr = eng.dev_alloc(flat.nbytes)
            try:
                eng.dev_upload(dptr, flat)
                eng.commit_batch_submit(0, dptr, n, 2, stride)
                got = eng.wait_batch(0, 2)
            finally:
                eng.dev_free(dptr)
            assert [g.compress() for g in got] == [sets[a][2], sets[b][2]], (sets[a][0], sets[b][0])
    finally:
        eng.set_max_batch(before)


CHILD = r"""
import json, os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "oracle"), %(tests)r]
import bigint_twin as T, kzg_poly_commit_exploration_amd as K, oracle_ctypes as O
import test_sort_single_recode_gpu as S
O.lib()
eng = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(S.N_MIN)
bad = []
try:
    cfg = eng.msm_config()
    for mont in (True, False):
        try:
            S.check_all(O, eng, S.N_MIN, mont)
        except AssertionError as e:
            bad.append(str(e)[:300])
finally:
    eng.close()
print(json.dumps({"bad": bad, "config": cfg}))
"""

KNOBS = [({"KZG_MSM_C": "15"}, ("windows", 15)), ({"KZG_MSM_C": "16"}, ("windows", 16)), ({"KZG_MSM_C": "17"}, ("windows", 17)),
         ({"KZG_MSM_C": "19"}, ("windows", 19)), ({"KZG_MSM_C": "13"}, ("windows", 13)),
         ({"KZG_MSM_RECODE": "naf", "KZG_MSM_C": "13"}, ("naf", 13)), ({"KZG_SPREAD_STAGED": "0"}, None),
         ({"KZG_SORT_PACKED": "0"}, None)]


def test_general_sort_under_its_switches():
    """one fresh process per setting, each with its own time limit; the first failure ends the test"""
    root = os.path.dirname(HERE)
    script = CHILD % {"root": root, "tests": HERE}
    for extra, want in KNOBS:
        env = dict(os.environ, **extra)
        p = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=120, env=env)
        assert p.returncode == 0, (extra, p.stdout[-2000:], p.stderr[-3000:])
        res = json.loads(p.stdout.strip().splitlines()[-1])
        assert res["bad"] == [], (extra, res["bad"])
        if want:
            assert (res["config"]["recoding"], res["config"]["digit_bits"]) == want, (extra, res["config"])
