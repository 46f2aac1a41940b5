"""GPU: multiproofs (kzg_open_points and friends) against the chained division over the C oracle (tests/open_points_oracle.py), the fixture and the single-point
entry points."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import kzg_poly_commit_exploration_amd as K
import open_points_oracle as PO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = K.R_MODULUS


def _rows(oracle, vals):
    return np.stack([oracle.fr_from_int(v) for v in vals])


def _case(oracle, n, k, seed):
    rnd = random.Random(seed)
    c = K.scalars_to_limbs([rnd.randrange(R) for _ in range(n)]) if n else np.zeros((0, 4), np.uint64)
    zs = [K.Scalar(rnd.randrange(R)) for _ in range(k)]
    ys = [K.Scalar.from_limbs(oracle.poly_evaluate(c, z.limbs())) for z in zs]
    return c, zs, ys


@pytest.fixture(scope="module")
def eng():
    e = K.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("n", [2, "k", "k+1", 2047, 2048, 2049, 4097, 70001, (1 << 20) + 1, (1 << 21) + 3 * 2048 + 5])
@pytest.mark.parametrize("k", [1, 2, 3, 16, 64])
def test_quotient_points_elementwise(eng, oracle, n, k):
    n = {"k": k, "k+1": k + 1}.get(n, n)
    if n > (1 << 21) and k > 3:
        pytest.skip("the block-stage launch is covered at k = 1, 2, 3 (the chained-division oracle is O(n k))")
    c, zs, ys = _case(oracle, n, k, n * 131 + k)
    rc, want = PO.quotient_points(oracle, c, np.stack([z.limbs() for z in zs]), np.stack([y.limbs() for y in ys]))
    assert rc == 0
    got = eng.quotient_points_limbs(c, zs, ys)
    assert got.shape == want.shape and np.array_equal(got, want)
    vals = eng.evaluate_points_limbs(c, zs)
    assert [v.v for v in vals] == [y.v for y in ys]
    for pos in sorted({0, k // 2, k - 1}):  # a wrong claim anywhere
        bad = list(ys)
        bad[pos] = K.Scalar(bad[pos].v + 1)
        with pytest.raises(K.KzgError) as ei:
            eng.quotient_points_limbs(c, zs, bad)
        assert ei.value.status == K.KZG_ERR_REMAINDER


def test_evaluate_points_equals_single_evaluations(eng, oracle):
    c, zs, _ = _case(oracle, 5000, 16, 3)
    assert [v.v for v in eng.evaluate_points_limbs(c, zs)] == [eng.evaluate_limbs(c, z).v for z in zs]


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "open_points.json")) as f:
        return json.load(f)


def test_proofs_against_fixture_and_oracle(engines, oracle, fixture):
    secret = bytes.fromhex(fixture["secret_be"])
    for cs in fixture["cases"]:
        n = cs["degree"] + 1
        e = engines.bench_srs(n)
        c = oracle.bench_coefficients(n)
        zs, ys = [K.Scalar(int(v, 16)) for v in cs["zs"]], [K.Scalar(int(v, 16)) for v in cs["ys"]]
        assert [v.v for v in e.evaluate_points_limbs(c, zs)] == [y.v for y in ys]
        pi = e.open_points_limbs(c, zs, ys)
        assert pi.compress().hex() == cs["proof"], (cs["degree"], cs["k"])
        if n <= 1 << 16:
            srs = oracle.srs_g1(n, secret)
            rc, want = PO.open_points(oracle, c, np.stack([z.limbs() for z in zs]), np.stack([y.limbs() for y in ys]), srs)
            assert rc == 0 and pi.compress() == oracle.p1_compress(want)


def test_k1_is_kzg_open_bit_for_bit(engines, oracle):
    for n in (2, 300, 4097, 70001):
        e = engines.bench_srs(max(n, 4097))
        c, zs, ys = _case(oracle, n, 1, n)
        a = e.open_points_limbs(c, zs, ys)
        b = e.open_limbs(c, zs[0], ys[0])
        assert np.array_equal(a.p1, b.p1)


def test_errors_and_low_degree(engines, oracle):
    srs_len = 4097
    e = engines.bench_srs(srs_len)
    k = 5
    # DEGREE_TOO_HIGH exactly at n' - k = srs_len + 1; n' - k = srs_len accepted
    for n, ok in ((srs_len + k, True), (srs_len + k + 1, False)):
        c, zs, ys = _case(oracle, n, k, n)
        if ok:
            pi = e.open_points_limbs(c, zs, ys)
            rc, q = PO.quotient_points(oracle, c, np.stack([z.limbs() for z in zs]), np.stack([y.limbs() for y in ys]))
            assert len(q) == srs_len
            srs = oracle.srs_g1(srs_len, bytes(range(32)))
            _, want = oracle.commit_pippenger(q, srs)
            assert pi.compress() == oracle.p1_compress(want)
        else:
            with pytest.raises(K.KzgError) as ei:
                e.open_points_limbs(c, zs, ys)
            assert ei.value.status == K.KZG_ERR_DEGREE_TOO_HIGH
            bad = list(ys)
            bad[2] = K.Scalar(bad[2].v + 1)
            with pytest.raises(K.KzgError) as ei:  # claims are checked first
                e.open_points_limbs(c, zs, bad)
            assert ei.value.status == K.KZG_ERR_REMAINDER
    c, zs, ys = _case(oracle, 100, 16, 9)
    for pos in (0, 8, 15):
        bad = list(ys)
        bad[pos] = K.Scalar(bad[pos].v + 1)
        with pytest.raises(K.KzgError) as ei:
            e.open_points_limbs(c, zs, bad)
        assert ei.value.status == K.KZG_ERR_REMAINDER
    for kk in (0, 65):
        with pytest.raises(K.KzgError) as ei:
            e.open_points_limbs(c, [K.Scalar(i + 1) for i in range(kk)], [K.Scalar(0)] * kk)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
    dup = [zs[0], zs[1], zs[0]]
    with pytest.raises(K.KzgError) as ei:
        e.open_points_limbs(c, dup, ys[:3])
    assert ei.value.status == K.KZG_ERR_INVALID_ARG
    # n' <= k with consistent claims: infinity; a constant polynomial follows the same rule
    for n in (0, 1, 3, 16):
        c, zs, ys = _case(oracle, n, 16, 50 + n)
        assert e.open_points_limbs(c, zs, ys).is_infinity()
        assert len(e.quotient_points_limbs(c, zs, ys)) == 0
    c = K.scalars_to_limbs([7])
    with pytest.raises(K.KzgError) as ei:
        e.open_points_limbs(c, [K.Scalar(3)], [K.Scalar(8)])
    assert ei.value.status == K.KZG_ERR_REMAINDER
    assert e.open_points_limbs(c, [K.Scalar(3)], [K.Scalar(7)]).is_infinity()


def test_submits_on_every_slot_interleaved(engines, oracle):
    n = 70001
    e = engines.bench_srs(n)
    slots = e.num_slots()
    jobs, ptrs = [], []
    try:
        for s in range(slots):
            c, zs, ys = _case(oracle, n, 1 + 7 * s, 1000 + s)
            d = e.dev_alloc(c.nbytes)
            ptrs.append(d)
            e.dev_upload(d, c)
            kind = s % 3
            if kind == 0:
                e.open_points_submit(s, d, n, zs, ys)
            elif kind == 1:
                e.commit_submit(s, d, n)
            else:
                e.open_submit(s, d, n, zs[0], ys[0])
            jobs.append((kind, c, zs, ys))
        for s, (kind, c, zs, ys) in enumerate(jobs):
            got = e.wait(s)
            if kind == 0:
                want = e.open_points_limbs(c, zs, ys)
            elif kind == 1:
                want = e.commit_limbs(c)
            else:
                want = e.open_limbs(c, zs[0], ys[0])
            assert np.array_equal(got.p1, want.p1), (s, kind)
        # a multiproof job's claims are checked at collection
        c, zs, ys = jobs[0][1], jobs[0][2], list(jobs[0][3])
        ys[0] = K.Scalar(ys[0].v + 1)
        e.open_points_submit(0, ptrs[0], n, zs, ys)
        with pytest.raises(K.KzgError) as ei:
            e.wait(0)
        assert ei.value.status == K.KZG_ERR_REMAINDER
    finally:
        for d in ptrs:
            e.dev_free(d)


def test_multi_device_contexts(oracle):
    import bigint_twin as T

    n = 3000
    c, zs, ys = _case(oracle, n, 4, 77)
    single = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(n)
    try:
        want = single.open_points_limbs(c, zs, ys)
    finally:
        single.close()
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(T.BENCH_SECRET_BE, n)
        assert np.array_equal(rep.open_points_limbs(c, zs, ys).p1, want.p1)
        assert [v.v for v in rep.evaluate_points_limbs(c, zs)] == [y.v for y in ys]
    finally:
        rep.close()
    rng = K.Engine(devices=[0, 0])
    try:
        rng.srs_generate(T.BENCH_SECRET_BE, n)
        with pytest.raises(K.KzgError) as ei:
            rng.open_points_limbs(c, zs, ys)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        assert b"not supported" in K.load_library().kzg_last_error(rng._h)
        assert len(rng.quotient_points_limbs(c, zs, ys)) == n - 4
    finally:
        rng.close()


def test_round_trip_commit_evaluate_open_verify_2_20(engines, oracle):
    import bigint_twin as T

    n = (1 << 20) + 1
    e = engines.bench_srs(n)
    c = oracle.bench_coefficients(n)
    zs = [K.Scalar(T.bench_input_point(n - 1) + 100 + i) for i in range(16)]
    cm = e.commit_limbs(c)
    ys = e.evaluate_points_limbs(c, zs)
    pi = e.open_points_limbs(c, zs, ys)
    g1 = e.srs_read(0, 16)
    g2 = np.stack([K.srs_g2_at(T.BENCH_SECRET_BE, j) for j in range(17)])
    assert K.verify_points(cm, pi, zs, ys, g1, g2)
    ys[3] = K.Scalar(ys[3].v + 1)
    assert not K.verify_points(cm, pi, zs, ys, g1, g2)


def test_example_open_points_runs():
    exe = os.path.join(ROOT, "examples", "open_points")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verified" in r.stdout
