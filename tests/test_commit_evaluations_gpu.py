"""GPU: kzg_commit_evaluations / kzg_open_evaluations against kzg_commit / kzg_open of the coefficients that
tests/ntt_oracle.py interpolates, and against the known-secret shortcut [P(s)]G with P(s) taken from the barycentric
formula on the values (no transform on that side)."""
import random

import numpy as np
import pytest

import bigint_twin as T
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu
R = NO.R
S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)


def _evals(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R) for _ in range(n)]


@pytest.mark.parametrize("k", [0, 1, 10, 16, 20])
def test_commit_evaluations_equals_commit_and_shortcut(engines, oracle, k):
    n = 1 << k
    eng = engines.bench_srs(max(n, 2))
    e = _evals(n, k)
    got = eng.commit_evaluations_limbs(K.scalars_to_limbs(e)).compress()
    assert got == eng.commit_limbs(K.scalars_to_limbs(NO.intt(e))).compress()
    assert got == TO.g1_scalar(oracle, NO.barycentric_eval(e, S))


def test_open_evaluations_inside_and_outside_the_domain(engines, oracle):
    k = 16
    n = 1 << k
    eng = engines.bench_srs(n)
    e = _evals(n, 77)
    a = K.scalars_to_limbs(e)
    c = K.scalars_to_limbs(NO.intt(e))
    commitment = eng.commit_evaluations_limbs(a)
    s_g2 = K.srs_g2_at(T.BENCH_SECRET_BE)
    w = NO.domain_root(k)
    for z, y in ((pow(w, 3, R), e[3]), (123456789, NO.barycentric_eval(e, 123456789))):
        zs, ys = K.Scalar(z), K.Scalar(y)
        proof = eng.open_evaluations_limbs(a, zs, ys)
        assert proof.compress() == eng.open_limbs(c, zs, ys).compress()
        assert proof.compress() == TO.proof(oracle, NO.intt(e), z, S, y)
        assert K.verify_proof(commitment, proof, zs, ys, s_g2)
        with pytest.raises(K.KzgError) as ei:
            eng.open_evaluations_limbs(a, zs, K.Scalar(y + 1))
        assert ei.value.status == K.KZG_ERR_REMAINDER


def test_submit_with_every_slot_in_flight(engines):
    n = 1 << 16
    eng = engines.bench_srs(n)
    slots = eng.num_slots()
    polys = [K.scalars_to_limbs(_evals(n, 500 + i)) for i in range(slots)]
    want = [eng.commit_evaluations_limbs(p).compress() for p in polys]
    bufs = [eng.dev_alloc(n * 32) for _ in range(slots)]
    try:
        for rnd in range(2):
            for i, (b, p) in enumerate(zip(bufs, polys)):
                eng.dev_upload(b, p)
            for i, b in enumerate(bufs):
                eng.commit_evaluations_submit(i, b, n)
            got = [eng.wait(i).compress() for i in range(slots)]
            assert got == want, rnd
    finally:
        for b in bufs:
            eng.dev_free(b)


def test_errors(engines):
    lib = K.load_library()
    eng = engines.bench_srs(1 << 10)
    small = K.scalars_to_limbs(_evals(4, 1))
    out = np.zeros(18, dtype=np.uint64)
    for n in (3, 0, 1 << 23):
        assert lib.kzg_commit_evaluations(eng._h, small.ctypes.data, n, out.ctypes.data) == K.KZG_ERR_INVALID_ARG, n
        assert lib.kzg_commit_evaluations_submit(eng._h, 0, 1, n) == K.KZG_ERR_INVALID_ARG, n
    # above the SRS length: full-degree values are refused, values of a low-degree polynomial are not (kzg_commit's rule)
    with pytest.raises(K.KzgError) as ei:
        eng.commit_evaluations_limbs(K.scalars_to_limbs(_evals(1 << 11, 2)))
    assert ei.value.status == K.KZG_ERR_DEGREE_TOO_HIGH
    low = NO.ntt(_evals(1 << 9, 3) + [0] * ((1 << 11) - (1 << 9)))
    assert eng.commit_evaluations_limbs(K.scalars_to_limbs(low)).compress() == \
        eng.commit_limbs(K.scalars_to_limbs(NO.intt(low))).compress()


def test_multi_device_contexts(oracle):
    n = 1 << 12
    e = K.scalars_to_limbs(_evals(n, 9))
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(T.BENCH_SECRET_BE, n)
        got = rep.commit_evaluations_limbs(e).compress()
        assert got == TO.g1_scalar(oracle, NO.barycentric_eval(K.limbs_to_scalars(e), S))
        z = K.Scalar(5)
        y = K.Scalar(NO.barycentric_eval(K.limbs_to_scalars(e), 5))
        assert rep.open_evaluations_limbs(e, z, y).compress() == \
            TO.proof(oracle, NO.intt(K.limbs_to_scalars(e)), 5, S, y.v)
    finally:
        rep.close()
    rng = K.Engine(devices=[0, 0])
    try:
        rng.srs_generate(T.BENCH_SECRET_BE, n)
        with pytest.raises(K.KzgError) as ei:
            rng.commit_evaluations_limbs(e)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        with pytest.raises(K.KzgError) as ei:
            rng.open_evaluations_limbs(e, K.Scalar(5), K.Scalar(1))
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        assert np.array_equal(rng.ntt_limbs(e), _oracle_ntt(e))
    finally:
        rng.close()


def _oracle_ntt(a):
    return K.scalars_to_limbs(NO.ntt(K.limbs_to_scalars(a)))


def test_polynomial_from_evaluations(engines):
    n = 1 << 8
    eng = engines.bench_srs(n)
    e = _evals(n, 11)
    p = K.Polynomial.from_evaluations(K.scalars_to_limbs(e), eng)
    assert K.limbs_to_scalars(p.limbs) == NO.intt(e)
    assert p.commit(eng).compress() == eng.commit_evaluations_limbs(K.scalars_to_limbs(e)).compress()
