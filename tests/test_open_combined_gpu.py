"""GPU: combined openings (kzg_open_combined and friends) against the big-integer restatement
(tests/open_combined_oracle.py), the single opening of the combined polynomial, and [v]G of the trapdoor oracle.

The coefficients are made and compared as blst_fr images (what the C-ABI carries): F, the values and the quotient are linear in
them, so the oracle works on the images directly; only the scalar of a proof takes the factor 2^256 out."""
import ctypes

import numpy as np
import pytest

import bigint_twin as T
import kzg_poly_commit_exploration_amd as K
import open_combined_oracle as CO
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu
R = K.R_MODULUS
RINV = CO.RINV
BENCH_S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)
KINDS = ("random", "max", "top")
NS = (1, 2, 255, 256, 257, 2047, 2048, 2049, 4097, 70001)  # lane, tile and finish-kernel boundaries
TS = (1, 2, 3, 17, 256)
GRID = [(n, t) for n in NS for t in TS if t < 256 or n <= 4097]


def _block(kind, n, t, seed):
    """(t, n, 4) uint64 images and the same as lists of integers"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 64, size=(t, n, 4), dtype=np.uint64)
    a[..., 3] = rng.integers(0, R >> 192, size=(t, n), dtype=np.uint64)  # below r
    if kind == "max":  # every image r - 1
        a[...] = CO.limbs_from_images([R - 1])[0]
    elif kind == "top":  # a single non-zero coefficient, the last one
        a[:, : n - 1] = 0
    return a, [CO.images_from_limbs(a[i]) for i in range(t)]


def _special(c, seed):
    """0, 1, r - 1 or a random scalar"""
    return (0, 1, R - 1, int(np.random.default_rng(seed).integers(1, 1 << 62)) * 0x9E3779B97F4A7C15F39CC0605CEDC835 % R)[c % 4]


def _value(image):
    return image * RINV % R


@pytest.fixture(scope="module")
def eng():
    e = K.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("n,t", GRID)
def test_hooks_elementwise(eng, n, t):
    """kzg_combine_polys and kzg_evaluate_batch_at against the oracle; the strides, the special values of gamma and z and the
    three kinds of coefficients rotate over the grid so that every combination of two of them occurs"""
    idx = GRID.index((n, t))
    kinds = KINDS if n * t <= 400000 else (KINDS[(n + t) % 3],)  # (the oracle is O(n t) big-integer steps)
    for kind in kinds:
        c = 3 * idx + KINDS.index(kind)
        gamma, z, stride = _special(c, c), _special(c // 4, c + 1000), n + 5 * ((c // 16) % 2)
        a, polys = _block(kind, n, t, c)
        f = eng.combine_polys_limbs(a, K.Scalar(gamma), stride=stride)
        assert np.array_equal(f, CO.limbs_from_images(CO.combine(polys, gamma))), (kind, gamma, stride)
        ys = eng.evaluate_batch_at_limbs(a, K.Scalar(z), stride=stride)
        assert [y.v for y in ys] == [_value(y) for y in CO.values(polys, z)], (kind, z, stride)


def test_hooks_do_not_depend_on_the_grouping(eng):
    n, t = 4099, 7
    a, polys = _block("random", n, t, 5)
    gamma, z = _special(3, 1), _special(3, 2)
    want_f, want_y = CO.limbs_from_images(CO.combine(polys, gamma)), [_value(y) for y in CO.values(polys, z)]
    before = eng.max_batch()
    try:
        for mb in (1, 3, t):
            eng.set_max_batch(mb)
            assert np.array_equal(eng.combine_polys_limbs(a, K.Scalar(gamma)), want_f), mb
            assert [y.v for y in eng.evaluate_batch_at_limbs(a, K.Scalar(z), stride=n + 5)] == want_y, mb
    finally:
        eng.set_max_batch(before)


# (n, t, extra stride, class of gamma, class of z, kind): the grid above thinned to a dozen
PROOF_CASES = [(1, 1, 0, 3, 3, "random"), (2, 2, 5, 3, 3, "random"), (255, 3, 0, 2, 3, "max"), (256, 17, 5, 3, 0, "random"),
               (257, 2, 0, 1, 1, "random"), (2047, 3, 5, 3, 2, "top"), (2048, 256, 0, 3, 3, "random"), (2049, 17, 5, 0, 3, "random"),
               (4097, 3, 0, 3, 3, "max"), (4097, 256, 5, 3, 1, "top"), (70001, 3, 5, 3, 3, "random"), (70001, 17, 0, 2, 3, "random")]


@pytest.mark.parametrize("n,t,extra,gc,zc,kind", PROOF_CASES)
def test_proof_is_the_opening_of_the_combined_polynomial(engines, oracle, n, t, extra, gc, zc, kind):
    e = engines.bench_srs(4097 if n <= 4097 else 70001)
    seed = 7 * n + t
    gamma, z = _special(gc, seed), _special(zc, seed + 1)
    a, polys = _block(kind, n, t, seed)
    ys, pi = e.open_combined_limbs(a, K.Scalar(z), K.Scalar(gamma), stride=n + extra)
    assert [y.v for y in ys] == [_value(y) for y in CO.values(polys, z)]
    f = CO.combine(polys, gamma)
    fz = TO.poly_eval(f, z)
    single = e.open_limbs(CO.limbs_from_images(f), K.Scalar(z), K.Scalar(_value(fz)))
    assert np.array_equal(pi.p1, single.p1)  # bit for bit
    assert pi.compress() == CO.proof(oracle, f, z, BENCH_S, images=True)


def test_same_bytes_by_every_route(engines, oracle):
    """the host-pointer call at three groupings and the resident submit / wait give the same bytes"""
    n, t = 4097, 7
    e = engines.bench_srs(4097)
    a, polys = _block("random", n, t, 11)
    gamma, z = K.Scalar(_special(3, 12)), K.Scalar(_special(3, 13))
    want_y = [_value(y) for y in CO.values(polys, z.v)]
    want_pi = CO.proof(oracle, CO.combine(polys, gamma.v), z.v, BENCH_S, images=True)
    got = []
    before = e.max_batch()
    try:
        for mb in (1, 3, t):
            e.set_max_batch(mb)
            ys, pi = e.open_combined_limbs(a, z, gamma)
            assert [y.v for y in ys] == want_y, mb
            got.append(pi.p1.tobytes())
    finally:
        e.set_max_batch(before)
    stride = n + 5
    block = np.zeros((t, stride, 4), dtype=np.uint64)
    block[:, :n] = a
    d = e.dev_alloc(block.nbytes)
    try:
        e.dev_upload(d, block)
        e.open_combined_submit(2, d, n, t, z, gamma, stride=stride)
        with pytest.raises(K.KzgError) as ei:  # kzg_wait does not collect it, and leaves it in the slot
            e.wait(2)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        ys, pi = e.wait_combined(2, t)
        assert [y.v for y in ys] == want_y
        got.append(pi.p1.tobytes())
        with pytest.raises(K.KzgError) as ei:  # the slot is idle again
            e.wait_combined(2, t)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
    finally:
        e.dev_free(d)
    assert len(set(got)) == 1 and K.G1Point(np.frombuffer(got[0], dtype=np.uint64)).compress() == want_pi


def test_one_polynomial_is_kzg_open_whatever_gamma(engines):
    e = engines.bench_srs(4097)
    for n in (2, 300, 4097):
        a, polys = _block("random", n, 1, n)
        z = _special(3, n)
        y = K.Scalar(_value(TO.poly_eval(polys[0], z)))
        want = e.open_limbs(a[0], K.Scalar(z), y)
        for gamma in (0, 1, _special(3, n + 1)):
            ys, pi = e.open_combined_limbs(a, K.Scalar(z), K.Scalar(gamma))
            assert ys[0].v == y.v and np.array_equal(pi.p1, want.p1), (n, gamma)


def test_cancellation(engines, oracle):
    e = engines.bench_srs(4097)
    n = 3000
    a, polys = _block("random", n, 2, 21)
    z = _special(3, 22)
    # P_1 = -P_0 and gamma = 1: F vanishes, the proof is infinity, the values are still returned
    neg = [[(-c) % R for c in polys[0]]]
    both = np.stack([a[0], CO.limbs_from_images(neg[0])])
    ys, pi = e.open_combined_limbs(both, K.Scalar(z), K.Scalar(1))
    y0 = TO.poly_eval(polys[0], z)
    assert [y.v for y in ys] == [_value(y0), _value(-y0 % R)] and pi.is_infinity() and not pi.p1.any()
    # F constant by cancellation: infinity as well, no constant-polynomial error
    const = [[(polys[0][0] + 5) % R] + neg[0][1:]]
    ys, pi = e.open_combined_limbs(np.stack([a[0], CO.limbs_from_images(const[0])]), K.Scalar(z), K.Scalar(1))
    assert pi.is_infinity() and ys[1].v == _value(TO.poly_eval(const[0], z))
    # the top coefficients cancel (n' = n - 40 < n): the proof is the one of the shorter F
    gamma = _special(3, 23)
    ginv = pow(gamma, -1, R)
    p1 = polys[1][: n - 40] + [(-c * ginv) % R for c in polys[0][n - 40:]]
    f = CO.combine([polys[0], p1], gamma)
    assert len(CO.truncate(f)) == n - 40
    ys, pi = e.open_combined_limbs(np.stack([a[0], CO.limbs_from_images(p1)]), K.Scalar(z), K.Scalar(gamma))
    assert pi.compress() == CO.proof(oracle, f, z, BENCH_S, images=True) and not pi.is_infinity()
    assert [y.v for y in ys] == [_value(y) for y in CO.values([polys[0], p1], z)]


def test_degree_against_an_srs_of_2048_points(engines, oracle):
    e = engines.bench_srs(2048)
    z = _special(3, 31)
    for n, ok in ((2049, True), (2050, False)):  # n' - 1 = 2048 fits, 2049 does not
        a, polys = _block("random", n, 2, n)
        gamma = _special(3, n + 1)
        if ok:
            ys, pi = e.open_combined_limbs(a, K.Scalar(z), K.Scalar(gamma))
            assert pi.compress() == CO.proof(oracle, CO.combine(polys, gamma), z, BENCH_S, images=True)
        else:
            with pytest.raises(K.KzgError) as ei:
                e.open_combined_limbs(a, K.Scalar(z), K.Scalar(gamma))
            assert ei.value.status == K.KZG_ERR_DEGREE_TOO_HIGH
            # the same polynomials pass once gamma makes the top coefficient cancel
            gamma = (-polys[0][n - 1]) * pow(polys[1][n - 1], -1, R) % R
            f = CO.combine(polys, gamma)
            assert len(CO.truncate(f)) == n - 1
            ys, pi = e.open_combined_limbs(a, K.Scalar(z), K.Scalar(gamma))
            assert pi.compress() == CO.proof(oracle, f, z, BENCH_S, images=True)
        assert [y.v for y in ys] == [_value(y) for y in CO.values(polys, z)]


def test_argument_errors(engines):
    e = engines.bench_srs(4097)
    lib = K.load_library()
    n, t = 100, 3
    a, _ = _block("random", n, t, 41)
    z, g = K.Scalar(5).limbs(), K.Scalar(7).limbs()
    ys, out = np.zeros((K.KZG_MAX_COMBINE + 1, 4), dtype=np.uint64), np.zeros(18, dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    call = lambda *args: lib.kzg_open_combined(e._h, *args)
    assert call(p(a), n, t, n, p(z), p(g), p(ys), p(out)) == K.KZG_OK
    assert call(p(a), n, 0, n, p(z), p(g), p(ys), p(out)) == K.KZG_ERR_INVALID_ARG
    assert call(p(a), n, K.KZG_MAX_COMBINE + 1, n, p(z), p(g), p(ys), p(out)) == K.KZG_ERR_INVALID_ARG
    assert call(p(a), n, t, n - 1, p(z), p(g), p(ys), p(out)) == K.KZG_ERR_INVALID_ARG  # stride < n with t > 1
    assert call(p(a), n, 1, 0, p(z), p(g), p(ys), p(out)) == K.KZG_OK  # (the stride of one polynomial is not read)
    for pos in (0, 4, 5, 6, 7):
        args = [p(a), n, t, n, p(z), p(g), p(ys), p(out)]
        args[pos] = None
        assert call(*args) == K.KZG_ERR_INVALID_ARG, pos
    not_fr = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    assert call(p(a), n, t, n, p(not_fr), p(g), p(ys), p(out)) == K.KZG_ERR_INVALID_ARG
    assert call(p(a), n, t, n, p(z), p(not_fr), p(ys), p(out)) == K.KZG_ERR_INVALID_ARG
    assert b"not below r" in lib.kzg_last_error(e._h)
    f = np.zeros((n, 4), dtype=np.uint64)
    assert lib.kzg_combine_polys(e._h, p(a), n, 0, n, p(g), p(f)) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_evaluate_batch_at(e._h, p(a), n, t, n - 1, p(z), p(ys)) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_open_combined_submit(e._h, 0, None, n, t, n, p(z), p(g)) == K.KZG_ERR_INVALID_ARG
    # no coefficients at all: every value is zero, the proof is infinity
    vals, pi = e.open_combined_limbs(np.zeros((2, 0, 4), dtype=np.uint64), K.Scalar(5), K.Scalar(7))
    assert [v.v for v in vals] == [0, 0] and pi.is_infinity()


def test_round_trip_commit_open_verify(engines):
    e = engines.bench_srs(4097)
    n, t = 4000, 5
    a, _ = _block("random", n, t, 51)
    z, gamma = K.Scalar(_special(3, 52)), K.Scalar(_special(3, 53))
    commitments = e.commit_batch_host(a)
    ys, pi = e.open_combined_limbs(a, z, gamma)
    s_g2 = K.srs_g2_at(T.BENCH_SECRET_BE, 1)
    assert K.verify_combined(commitments, ys, z, gamma, pi, s_g2)
    c, y = K.combine_claims(commitments, ys, gamma)
    assert K.verify_proof_batch([c], [pi], [z], [y], s_g2) == [True]
    bad = list(ys)
    bad[2] = K.Scalar(bad[2].v + 1)
    assert not K.verify_combined(commitments, bad, z, gamma, pi, s_g2)


def test_full_size_once(engines, oracle):
    """n = 2^20, t = 3 on resident inputs: the proof is [v]G for v = (F(s) - F(z)) / (s - z), F(x) = sum gamma^i P_i(x)"""
    n, t = 1 << 20, 3
    e = engines.bench_srs((1 << 20) + 1)
    a, polys = _block("random", n, t, 61)
    gamma, z = _special(3, 62), _special(3, 63)
    d = e.dev_alloc(a.nbytes)
    try:
        e.dev_upload(d, a)
        e.open_combined_submit(0, d, n, t, K.Scalar(z), K.Scalar(gamma))
        at_z, at_s = CO.values(polys, z), CO.values(polys, BENCH_S)  # (while the device works)
        ys, pi = e.wait_combined(0, t)
    finally:
        e.dev_free(d)
    assert [y.v for y in ys] == [_value(y) for y in at_z]
    _, fz = CO.combined_claim([0] * t, at_z, gamma)
    _, fs = CO.combined_claim([0] * t, at_s, gamma)
    v = (fs - fz) * pow(BENCH_S - z, -1, R) % R
    assert pi.compress() == TO.g1_scalar(oracle, _value(v))


def test_multi_device_contexts(oracle):
    n, t = 3000, 4
    a, polys = _block("random", n, t, 71)
    z, gamma = K.Scalar(_special(3, 72)), K.Scalar(_special(3, 73))
    want_y = [_value(y) for y in CO.values(polys, z.v)]
    want_pi = CO.proof(oracle, CO.combine(polys, gamma.v), z.v, BENCH_S, images=True)
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(T.BENCH_SECRET_BE, n)
        ys, pi = rep.open_combined_limbs(a, z, gamma)
        assert [y.v for y in ys] == want_y and pi.compress() == want_pi
        assert [y.v for y in rep.evaluate_batch_at_limbs(a, z)] == want_y
    finally:
        rep.close()
    rng = K.Engine(devices=[0, 0])
    try:
        rng.srs_generate(T.BENCH_SECRET_BE, n)
        with pytest.raises(K.KzgError) as ei:
            rng.open_combined_limbs(a, z, gamma)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        assert b"not supported" in K.load_library().kzg_last_error(rng._h)
        assert [y.v for y in rng.evaluate_batch_at_limbs(a, z)] == want_y
        assert np.array_equal(rng.combine_polys_limbs(a, gamma), CO.limbs_from_images(CO.combine(polys, gamma.v)))
    finally:
        rng.close()


def test_example_open_combined_runs():
    import os
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "open_combined")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verified" in r.stdout
