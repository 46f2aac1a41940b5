"""The quotient scans (poly_kernels.hip) at special points: z = 0 (division by X: every power of z but z^0 is zero),
z = 1, z = r - 1, and roots of unity with z^L = 1 for the chunk lengths kPolyL = 8 and kPolySingleL = 16, so that the
chunk, block and carry multipliers (powers of z) collapse to 0 or 1.  Sizes cover every scan form: 2 and 4096
(k_poly_single), 4097 and 2^20 + 1 (direct carries), 2^21 + 2049 (block stage).  Multiproofs at point sets with 0, +-z
pairs, consecutive integers and roots of unity.  References: oracle.quotient / open_points_oracle elementwise, the
trapdoor oracle (tests/trapdoor_oracle.py) for the proofs."""
import random

import numpy as np
import pytest

import bigint_twin as T
import kzg_poly_commit_exploration_amd as K
import open_points_oracle as PO
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu

R = TO.R
BENCH_S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)
N20 = (1 << 20) + 1
N_BLOCK = (1 << 21) + 2049
ROOT8 = pow(7, (R - 1) >> 3, R)    # z^8 = 1: z^kPolyL = 1
ROOT16 = pow(7, (R - 1) >> 4, R)   # z^16 = 1: z^kPolySingleL = 1
POINTS = {"0": 0, "1": 1, "r-1": R - 1, "root8": ROOT8, "root16": ROOT16}

_poly = {}


def poly(n):
    """prefix of one uniform polynomial of N_BLOCK terms: (values, limbs)"""
    if not _poly:
        rng = random.Random(2049)
        vals = [rng.randrange(R) for _ in range(N_BLOCK)]
        _poly["v"], _poly["l"] = vals, K.scalars_to_limbs(vals)
    return _poly["v"][:n], np.ascontiguousarray(_poly["l"][:n])


@pytest.fixture(scope="module")
def bare():
    e = K.Engine(0)
    yield e
    e.close()


def test_roots_are_primitive():
    assert pow(ROOT8, 8, R) == 1 and pow(ROOT8, 4, R) != 1
    assert pow(ROOT16, 16, R) == 1 and pow(ROOT16, 8, R) != 1


@pytest.mark.parametrize("n", [2, 4096, 4097, N20, N_BLOCK])
@pytest.mark.parametrize("zname", sorted(POINTS))
def test_quotient_at_special_points(engines, bare, oracle, n, zname):
    z = POINTS[zname]
    vals, c = poly(n)
    zm = oracle.fr_from_int(z)
    ym = oracle.poly_evaluate(c, zm)
    y = oracle.fr_to_int(ym)
    eng = bare if n > N20 else engines.bench_srs(4097 if n <= 4097 else N20)
    assert eng.evaluate_limbs(c, K.Scalar(z)).v == y
    rc, q_want = oracle.quotient(c, zm, ym)
    assert rc == 0
    q_got = eng.quotient_limbs(c, K.Scalar(z), K.Scalar(y))
    assert q_got.shape == q_want.shape and np.array_equal(q_got, q_want), (n, zname)
    if n <= N20:
        got = eng.open_limbs(c, K.Scalar(z), K.Scalar(y)).compress()
        assert got == TO.proof(oracle, vals, z, BENCH_S, y), (n, zname)
    with pytest.raises(K.KzgError) as ei:
        eng.quotient_limbs(c, K.Scalar(z), K.Scalar(y + 1))
    assert ei.value.status == K.KZG_ERR_REMAINDER


def _point_sets():
    rng = random.Random(64)
    pairs = []
    for _ in range(4):
        z = rng.randrange(R)
        pairs += [z, R - z]
    return {"0,1,r-1": [0, 1, R - 1], "+-z": pairs, "64 consecutive": list(range(1000, 1064)),
            "8th roots": [pow(ROOT8, i, R) for i in range(8)], "16th roots": [pow(ROOT16, i, R) for i in range(16)],
            "0 and 16th roots": [0] + [pow(ROOT16, i, R) for i in range(16)]}


@pytest.mark.parametrize("n", [4097, N20])
@pytest.mark.parametrize("pset", sorted(_point_sets()))
def test_multiproof_at_special_point_sets(engines, oracle, n, pset):
    zs = _point_sets()[pset]
    vals, c = poly(n)
    zrows = oracle.fr_from_ints(zs)
    yrows = np.stack([oracle.poly_evaluate(c, zr) for zr in zrows])
    ys = [oracle.fr_to_int(r) for r in yrows]
    eng = engines.bench_srs(4097 if n <= 4097 else N20)
    rc, q_want = PO.quotient_points(oracle, c, zrows, yrows)
    assert rc == 0
    q_got = eng.quotient_points_limbs(c, [K.Scalar(z) for z in zs], [K.Scalar(y) for y in ys])
    assert q_got.shape == q_want.shape and np.array_equal(q_got, q_want), (n, pset)
    got = eng.open_points_limbs(c, [K.Scalar(z) for z in zs], [K.Scalar(y) for y in ys]).compress()
    assert got == TO.multiproof(oracle, vals, zs, BENCH_S, ys), (n, pset)
