"""CPU: multiproofs (one proof for P at k points) -- the chained division over the C oracle (tests/open_points_oracle.py)
against big-int long division, the fixture against the oracle, and the host verifier kzg_verify_points against the fixture
and the pairing twin."""
import json
import os
import random

import numpy as np
import pytest

import kzg_poly_commit_exploration_amd as K
import open_points_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = K.R_MODULUS


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "open_points.json")) as f:
        return json.load(f)


def _rows(oracle, vals):
    return np.stack([oracle.fr_from_int(v) for v in vals])


@pytest.mark.parametrize("n,k", [(0, 1), (1, 1), (1, 3), (3, 3), (4, 3), (5, 2), (9, 1), (17, 5), (40, 8), (8, 40)])
def test_oracle_quotient_points_against_twin(oracle, twin, n, k):
    rnd = random.Random(n * 100 + k)
    c = [rnd.randrange(R) for _ in range(n)]
    zs = [rnd.randrange(R) for _ in range(k)]
    ys = [twin.poly_evaluate(c, z) for z in zs]
    q_twin, rem = PO.poly_div_vanishing(c, zs)
    rc, q = PO.quotient_points(oracle, _rows(oracle, c) if n else np.zeros((0, 4), np.uint64), _rows(oracle, zs), _rows(oracle, ys))
    assert rc == 0
    assert [oracle.fr_to_int(r) for r in q] == q_twin
    assert len(q_twin) == max(len([1 for i, x in enumerate(c) if any(y % R for y in c[i:])]) - k, 0)
    # q * Z + I = P
    zc = [1]
    for z in zs:
        zc = [((zc[j - 1] if j else 0) - z * (zc[j] if j < len(zc) else 0)) % R for j in range(len(zc) + 1)]
    back = [0] * max(n, len(q_twin) + k, 1)
    for i, a in enumerate(q_twin):
        for j, b in enumerate(zc):
            back[i + j] = (back[i + j] + a * b) % R
    for i, a in enumerate(rem):
        back[i] = (back[i] + a) % R
    strip = lambda v: v[: max([i + 1 for i, x in enumerate(v) if x % R] + [0])]  # noqa: E731
    assert strip(back) == strip([x % R for x in c])
    for i, z in enumerate(zs):  # the interpolant takes the claims
        assert twin.poly_evaluate(rem, z) == ys[i]
    if k and n:
        bad = list(ys)
        bad[k // 2] = (bad[k // 2] + 1) % R
        rc, _ = PO.quotient_points(oracle, _rows(oracle, c), _rows(oracle, zs), _rows(oracle, bad))
        assert rc == K.KZG_ERR_REMAINDER  # (the oracle's codes mirror the library's)


def test_fixture_small_degree_against_oracle(oracle, fixture):
    secret = bytes.fromhex(fixture["secret_be"])
    for cs in fixture["cases"]:
        if cs["degree"] != 1 << 10:
            continue
        n = cs["degree"] + 1
        c = oracle.bench_coefficients(n)
        zs, ys = [int(v, 16) for v in cs["zs"]], [int(v, 16) for v in cs["ys"]]
        for z, y in zip(zs, ys):
            assert oracle.fr_to_int(oracle.poly_evaluate(c, oracle.fr_from_int(z))) == y
        srs = oracle.srs_g1(n, secret)
        rc, pt = PO.open_points(oracle, c, _rows(oracle, zs), _rows(oracle, ys), srs)
        assert rc == 0
        assert oracle.p1_compress(pt).hex() == cs["proof"]
        rc, cm = oracle.commit_pippenger(c, srs)
        assert oracle.p1_compress(cm).hex() == cs["commitment"]


def _setup(oracle, secret, k):
    g1 = oracle.srs_g1(max(k, 1), secret)
    g2 = np.stack([K.srs_g2_at(secret, j) for j in range(k + 1)])
    return g1, g2


def _scalars(vals):
    return [K.Scalar(v) for v in vals]


@pytest.mark.parametrize("k", [2, 16, 64])
def test_verify_points_accepts_fixture_and_rejects_tampering(oracle, fixture, k):
    secret = bytes.fromhex(fixture["secret_be"])
    g1, g2 = _setup(oracle, secret, k)
    for cs in fixture["cases"]:
        if cs["k"] != k:
            continue
        C = K.G1Point.uncompress(bytes.fromhex(cs["commitment"]))
        pi = K.G1Point.uncompress(bytes.fromhex(cs["proof"]))
        zs, ys = [int(v, 16) for v in cs["zs"]], [int(v, 16) for v in cs["ys"]]
        assert K.verify_points(C, pi, _scalars(zs), _scalars(ys), g1, g2)
        if cs["degree"] != 1 << 10:
            continue
        bad_y = list(ys)
        bad_y[-1] = (bad_y[-1] + 1) % R
        assert not K.verify_points(C, pi, _scalars(zs), _scalars(bad_y), g1, g2)
        bad_z = list(zs)
        bad_z[0] = (bad_z[0] + 1000) % R
        assert not K.verify_points(C, pi, _scalars(bad_z), _scalars(ys), g1, g2)
        swapped = [zs[1], zs[0]] + zs[2:]  # points swapped, claims kept in place
        assert not K.verify_points(C, pi, _scalars(swapped), _scalars(ys), g1, g2)
        other = K.G1Point(oracle.p1_generator())
        assert not K.verify_points(C, other, _scalars(zs), _scalars(ys), g1, g2)
        assert not K.verify_points(other, pi, _scalars(zs), _scalars(ys), g1, g2)


def test_verify_points_at_k1_agrees_with_verify_proof(oracle, twin):
    secret = twin.BENCH_SECRET_BE
    n = 33
    c = oracle.bench_coefficients(n)
    z = oracle.bench_input_point(n - 1)
    y = oracle.poly_evaluate(c, z)
    srs = oracle.srs_g1(n, secret)
    rc, proof = oracle.generate_proof(c, z, y, srs)
    assert rc == 0
    _, cm = oracle.commit_naive(c, srs)
    g2 = np.stack([K.srs_g2_at(secret, j) for j in range(2)])
    C, pi = K.G1Point(cm), K.G1Point(proof)
    zs, ys = [K.Scalar.from_limbs(z)], [K.Scalar.from_limbs(y)]
    for yy in (ys, [K.Scalar(ys[0].v + 1)]):
        assert K.verify_points(C, pi, zs, yy, srs, g2) == K.verify_proof(C, pi, zs[0], yy[0], g2[1])
    assert K.verify_points(C, pi, zs, ys, srs, g2)


def test_verify_points_agrees_with_pairing_twin(oracle, twin):
    secret = twin.BENCH_SECRET_BE
    rnd = random.Random(7)
    n, k = 12, 3
    c = [rnd.randrange(R) for _ in range(n)]
    zs = [rnd.randrange(R) for _ in range(k)]
    ys = [twin.poly_evaluate(c, z) for z in zs]
    srs_t = twin.srs_g1(secret, n)
    q, _ = PO.poly_div_vanishing(c, zs)
    C_t, pi_t = twin.commit_naive(c, srs_t), twin.commit_naive(q, srs_t)
    g1, g2 = _setup(oracle, secret, k)
    C = K.G1Point(np.array(twin.g1_to_blst_p1_limbs(C_t), dtype=np.uint64))
    pi = K.G1Point(np.array(twin.g1_to_blst_p1_limbs(pi_t), dtype=np.uint64))
    for claims in (ys, [ys[0], (ys[1] + 1) % R, ys[2]]):
        assert K.verify_points(C, pi, _scalars(zs), _scalars(claims), g1, g2) == PO.verify_points(C_t, pi_t, zs, claims, secret)
    assert PO.verify_points(C_t, pi_t, zs, ys, secret)


def test_verify_points_refuses_malformed_inputs(oracle, twin):
    secret = twin.BENCH_SECRET_BE
    g1, g2 = _setup(oracle, secret, 3)
    G = K.G1Point(oracle.p1_generator())
    zs, ys = _scalars([1, 2, 3]), _scalars([4, 5, 6])
    with pytest.raises(K.KzgError) as ei:  # two equal points
        K.verify_points(G, G, _scalars([1, 2, 1]), ys, g1, g2)
    assert ei.value.status == K.KZG_ERR_INVALID_ARG
    off = g2.copy()
    off[2, 0] ^= np.uint64(1)  # x of [s^2]G2 moved off the twist
    with pytest.raises(K.KzgError) as ei:
        K.verify_points(G, G, zs, ys, g1, off)
    assert ei.value.status == K.KZG_ERR_INVALID_ARG
    bad1 = g1.copy()
    bad1[1, 0] ^= np.uint64(1)  # an SRS G1 entry off the curve
    with pytest.raises(K.KzgError) as ei:
        K.verify_points(G, G, zs, ys, bad1, g2)
    assert ei.value.status == K.KZG_ERR_INVALID_ARG
