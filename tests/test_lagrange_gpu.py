"""GPU: the Lagrange basis kept by the context and the calls on values over it -- kzg_lagrange_*,
kzg_commit_lagrange*, kzg_open_lagrange*, kzg_quotient_lagrange, the two loaders of a basis given as bytes.  Every comparison
is bit for bit: against tests/lagrange_oracle.py and the known-secret shortcuts of tests/trapdoor_oracle.py, and against the
coefficient route (kzg_commit_evaluations / kzg_open_evaluations) on the same input, statuses included.

Sizes are the smallest that reach each path: n = 1, 2, 4 (below one lane's run of four), 1024 (one tile of the quotient
kernel), 2048 (two tiles: the cross-tile sums), 4096 (the one-launch small MSM, 65536 references), 2^14 (the general sort /
accumulate / tail path)."""
import random

import numpy as np
import pytest

import bigint_twin as T
import kzg_poly_commit_exploration_amd as K
import lagrange_oracle as LO
import ntt_oracle as NO
import oracle_ctypes as O
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu
R = NO.R
S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)
SIZES = [1, 2, 4, 1024, 2048, 4096, 1 << 14]
INF48 = bytes([0xC0]) + bytes(47)
OFF_CURVE48 = bytes([0x80]) + bytes(46) + bytes([0x01])  # x = 1 is not on the curve


def _evals(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R) for _ in range(n)]


def _compress_rows(rows):
    return [O.p1_compress(r) for r in np.asarray(rows, dtype=np.uint64).reshape(-1, 18)]


def _status(fn):
    """(status, compressed point or None)"""
    try:
        return K.KZG_OK, fn().compress()
    except K.KzgError as e:
        return e.status, None


_BASIS = {}  # (log_n, secret) -> the expected compressed points, computed once


def _expected_basis(oracle, log_n, s=S):
    if (log_n, s) not in _BASIS:
        _BASIS[(log_n, s)] = [TO.g1_scalar(oracle, l) for l in LO.lagrange_at(log_n, s)]
    return _BASIS[(log_n, s)]


_CASES = {}  # n -> (values, limbs, coefficients): one set per size, shared and left unchanged


def _case(n):
    if n not in _CASES:
        e = _evals(n, 7000 + n)
        _CASES[n] = (e, K.scalars_to_limbs(e), NO.intt(e))
    return _CASES[n]


def _in_domain(n):
    ms = {0, n - 1, n // 2}
    if n == 2048:
        ms |= {1023, 1024}  # the last index of the first tile and the first of the second
    return sorted(ms)


# ---- the basis ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [0, 1, 2, 5, 10, 12])
def test_basis_points_equal_the_oracle(engines, oracle, log_n):
    n = 1 << log_n
    want = _expected_basis(oracle, log_n)
    for srs_len in (n, 1 << 14):  # an SRS of exactly n points, and a longer one
        eng = engines.bench_srs(srs_len)
        eng.lagrange_prepare(log_n)
        assert eng.lagrange_len() == n
        assert _compress_rows(eng.lagrange_read(0, n)) == want, srs_len
        assert _compress_rows(eng.lagrange_read(n - 1, 1)) == want[n - 1:]
    lib = K.load_library()
    eng = engines.bench_srs(n)
    out = np.zeros((2, 18), dtype=np.uint64)
    assert lib.kzg_lagrange_read_g1(eng._h, n, 1, out.ctypes.data) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_lagrange_prepare(eng._h, log_n + 1) == K.KZG_ERR_DEGREE_TOO_HIGH
    assert lib.kzg_lagrange_prepare(eng._h, K.KZG_NTT_MAX_LOG + 1) == K.KZG_ERR_INVALID_ARG
    assert eng.lagrange_len() == n  # a refused request leaves the held basis


def test_no_srs_no_basis():
    lib = K.load_library()
    eng = K.Engine(0)
    try:
        out = np.zeros(18, dtype=np.uint64)
        assert lib.kzg_lagrange_prepare(eng._h, 3) == K.KZG_ERR_NO_SRS
        assert eng.lagrange_len() == 0
        assert lib.kzg_lagrange_read_g1(eng._h, 0, 1, out.ctypes.data) == K.KZG_ERR_NO_SRS
        a = K.scalars_to_limbs(_evals(4, 1))
        assert lib.kzg_commit_lagrange(eng._h, a.ctypes.data, 4, out.ctypes.data) == K.KZG_ERR_NO_SRS
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["one", "w3", "minus_one", "zero"])
def test_degenerate_setups(oracle, name):
    """s in the domain: the basis is G at one index and infinity elsewhere; s = 0: [1/n]G everywhere"""
    n, k = 64, 6
    w = NO.domain_root(k)
    s = {"one": 1, "w3": pow(w, 3, R), "minus_one": R - 1, "zero": 0}[name]
    eng = K.SetupArtifactsGenerator(TO.secret_be(s)).take(n)
    try:
        eng.lagrange_prepare(k)
        got = _compress_rows(eng.lagrange_read(0, n))
        if name == "zero":
            assert got == [TO.g1_scalar(oracle, pow(n, R - 2, R))] * n
        else:
            m = {"one": 0, "w3": 3, "minus_one": 32}[name]
            assert got == [TO.g1_scalar(oracle, 1) if i == m else INF48 for i in range(n)]
        e = _evals(n, 64)
        a = K.scalars_to_limbs(e)
        c = eng.commit_lagrange_limbs(a).compress()
        assert c == eng.commit_evaluations_limbs(a).compress()
        assert c == TO.g1_scalar(oracle, NO.barycentric_eval(e, s))
    finally:
        eng.close()


# ---- commitments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_commit_equals_the_coefficient_route_and_the_shortcut(engines, oracle, n):
    eng = engines.bench_srs(n)
    e, a, _ = _case(n)
    got = eng.commit_lagrange_limbs(a).compress()  # builds the basis on first use
    assert eng.lagrange_len() == n
    assert got == eng.commit_evaluations_limbs(a).compress()
    assert got == TO.g1_scalar(oracle, NO.barycentric_eval(e, S))


@pytest.mark.parametrize("n", [4, 2048, 1 << 14])
def test_commit_structured_values(engines, oracle, n):
    eng = engines.bench_srs(n)
    k = NO.log2_exact(n)
    eng.lagrange_prepare(k)
    commit = lambda vals: eng.commit_lagrange_limbs(K.scalars_to_limbs(vals)).compress()
    assert commit([0] * n) == INF48
    v = 0x1234567890ABCDEF
    assert commit([v] * n) == TO.g1_scalar(oracle, v)  # the basis sums to G
    assert commit([R - 1] * n) == TO.g1_scalar(oracle, R - 1)
    ls = LO.lagrange_at(k, S)
    for at in (0, n // 2, n - 1):  # one non-zero value: the scaled basis point
        assert commit([v if i == at else 0 for i in range(n)]) == TO.g1_scalar(oracle, v * ls[at]), at


def test_commit_errors(engines):
    lib = K.load_library()
    eng = engines.bench_srs(1024)
    eng.lagrange_prepare(10)
    a = K.scalars_to_limbs(_evals(2048, 3))
    out = np.zeros(18, dtype=np.uint64)
    assert lib.kzg_commit_lagrange(eng._h, a.ctypes.data, 2048, out.ctypes.data) == K.KZG_ERR_DEGREE_TOO_HIGH
    assert lib.kzg_commit_lagrange_submit(eng._h, 0, a.ctypes.data, 2048) == K.KZG_ERR_DEGREE_TOO_HIGH
    z = K.Scalar(5).limbs()
    assert lib.kzg_open_lagrange(eng._h, a.ctypes.data, 2048, z.ctypes.data, z.ctypes.data, out.ctypes.data) == \
        K.KZG_ERR_DEGREE_TOO_HIGH
    for n in (3, 0, 1 << 23):
        assert lib.kzg_commit_lagrange(eng._h, a.ctypes.data, n, out.ctypes.data) == K.KZG_ERR_INVALID_ARG, n
        assert lib.kzg_commit_lagrange_submit(eng._h, 0, a.ctypes.data, n) == K.KZG_ERR_INVALID_ARG, n
        assert lib.kzg_commit_lagrange_batch(eng._h, a.ctypes.data, n, 1, 1 << 23, out.ctypes.data) == K.KZG_ERR_INVALID_ARG, n
        assert lib.kzg_open_lagrange(eng._h, a.ctypes.data, n, z.ctypes.data, z.ctypes.data, out.ctypes.data) == \
            K.KZG_ERR_INVALID_ARG, n
        assert lib.kzg_quotient_lagrange(eng._h, a.ctypes.data, n, z.ctypes.data, z.ctypes.data, a.ctypes.data) == \
            K.KZG_ERR_INVALID_ARG, n
    assert eng.lagrange_len() == 1024


# ---- the pipeline ------------------------------------------------------------------------------------------------------------
def test_submit_alternating_with_the_monomial_table(engines):
    """every slot in flight for two rounds, Lagrange and monomial jobs alternating: both tables are read by jobs in flight together"""
    n = 1 << 14
    eng = engines.bench_srs(n)
    eng.lagrange_prepare(14)
    slots = eng.num_slots()
    polys = [K.scalars_to_limbs(_evals(n, 900 + i)) for i in range(slots)]
    want_l = [eng.commit_lagrange_limbs(p).compress() for p in polys]
    want_m = [eng.commit_limbs(p).compress() for p in polys]
    bufs = [eng.dev_alloc(n * 32) for _ in range(slots)]
    try:
        for b, p in zip(bufs, polys):
            eng.dev_upload(b, p)
        for rnd in range(2):
            lag = [(i + rnd) % 2 == 0 for i in range(slots)]
            for i, b in enumerate(bufs):
                (eng.commit_lagrange_submit if lag[i] else eng.commit_submit)(i, b, n)
            got = [eng.wait(i).compress() for i in range(slots)]
            assert got == [want_l[i] if lag[i] else want_m[i] for i in range(slots)], rnd
        # the submit calls never build: no basis of exactly n -> KZG_ERR_NO_SRS
        lib = K.load_library()
        eng.lagrange_prepare(13)
        z = K.Scalar(5).limbs()
        assert lib.kzg_commit_lagrange_submit(eng._h, 0, bufs[0], n) == K.KZG_ERR_NO_SRS
        assert lib.kzg_open_lagrange_submit(eng._h, 0, bufs[0], n, z.ctypes.data, z.ctypes.data) == K.KZG_ERR_NO_SRS
        assert eng.lagrange_len() == 1 << 13
    finally:
        for b in bufs:
            eng.dev_free(b)
    fresh = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(1024)  # an SRS and no basis at all
    try:
        d = fresh.dev_alloc(1024 * 32)
        assert K.load_library().kzg_commit_lagrange_submit(fresh._h, 0, d, 1024) == K.KZG_ERR_NO_SRS
        fresh.dev_free(d)
    finally:
        fresh.close()


def test_batch_with_a_stride_under_two_batch_limits(engines):
    n, batch, stride = 1 << 14, 5, (1 << 14) + 3
    eng = engines.bench_srs(n)
    rows = np.zeros((batch, stride, 4), dtype=np.uint64)
    for b in range(batch):
        rows[b] = K.scalars_to_limbs(_evals(stride, 950 + b))  # the values past n are not the polynomial's
    want = [eng.commit_lagrange_limbs(rows[b, :n]).compress() for b in range(batch)]
    before = eng.max_batch()
    try:
        for mb in (1, 4):
            eng.set_max_batch(mb)
            assert eng.lagrange_len() == n  # resizing the workspaces keeps the basis
            assert [p.compress() for p in eng.commit_lagrange_batch(rows, n=n)] == want, mb
    finally:
        eng.set_max_batch(before)


# ---- openings ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_open_equals_the_coefficient_route_and_the_shortcut(engines, oracle, n):
    eng = engines.bench_srs(n)
    e, a, c = _case(n)
    k = NO.log2_exact(n)
    w = NO.domain_root(k)
    commitment = eng.commit_lagrange_limbs(a)
    s_g2 = K.srs_g2_at(T.BENCH_SECRET_BE)
    points = [(0xABCDEF0123456789 + n, None), (0, None)] + [(pow(w, m, R), m) for m in _in_domain(n)]
    for z, m in points:
        y = e[m] if m is not None else TO.poly_eval(c, z)
        zs, ys = K.Scalar(z), K.Scalar(y)
        got = _status(lambda: eng.open_lagrange_limbs(a, zs, ys))
        assert got == _status(lambda: eng.open_evaluations_limbs(a, zs, ys)), (z, m)
        if n == 1:  # a constant: infinity for the value itself
            assert got == (K.KZG_OK, INF48)
        else:
            assert got == (K.KZG_OK, TO.proof(oracle, c, z, S, y)), (z, m)
            assert K.verify_proof(commitment, eng.open_lagrange_limbs(a, zs, ys), zs, ys, s_g2)
        bad = K.Scalar(y + 1)  # a wrong claim, inside and outside the domain
        got = _status(lambda: eng.open_lagrange_limbs(a, zs, bad))
        assert got == _status(lambda: eng.open_evaluations_limbs(a, zs, bad)), (z, m)
        assert got[0] == (K.KZG_ERR_CONSTANT_POLY if n == 1 else K.KZG_ERR_REMAINDER)


@pytest.mark.parametrize("n", [1, 4, 2048])
def test_open_constant_values(engines, n):
    eng = engines.bench_srs(n)
    v = 0xFEDCBA9876543210
    a = K.scalars_to_limbs([v] * n)
    w = NO.domain_root(NO.log2_exact(n))
    for z in (12345, pow(w, n - 1, R)):
        for y, want in ((v, (K.KZG_OK, INF48)), (v + 1, (K.KZG_ERR_CONSTANT_POLY, None))):
            got = _status(lambda: eng.open_lagrange_limbs(a, K.Scalar(z), K.Scalar(y)))
            assert got == want == _status(lambda: eng.open_evaluations_limbs(a, K.Scalar(z), K.Scalar(y))), (z, y)


def test_open_submit_with_every_slot_in_flight(engines, oracle):
    n = 1 << 14
    eng = engines.bench_srs(n)
    eng.lagrange_prepare(14)
    slots = eng.num_slots()
    w = NO.domain_root(14)
    evals = [_evals(n, 1200 + i) for i in range(slots)]
    zs = [pow(w, 16383 * i, R) if i % 2 else 1000 + i for i in range(slots)]  # in the domain and outside it
    ys = [NO.barycentric_eval(e, z) for e, z in zip(evals, zs)]
    want = [eng.open_evaluations_limbs(K.scalars_to_limbs(e), K.Scalar(z), K.Scalar(y)).compress() for e, z, y in zip(evals, zs, ys)]
    bufs = [eng.dev_alloc(n * 32) for _ in range(slots)]
    try:
        for b, e in zip(bufs, evals):
            eng.dev_upload(b, K.scalars_to_limbs(e))
        for rnd in range(2):
            for i, b in enumerate(bufs):
                eng.open_lagrange_submit(i, b, n, K.Scalar(zs[i]), K.Scalar(ys[i]))
            assert [eng.wait(i).compress() for i in range(slots)] == want, rnd
        eng.open_lagrange_submit(0, bufs[0], n, K.Scalar(zs[0]), K.Scalar(ys[0] + 1))
        with pytest.raises(K.KzgError) as ei:
            eng.wait(0)
        assert ei.value.status == K.KZG_ERR_REMAINDER
    finally:
        for b in bufs:
            eng.dev_free(b)


# ---- the quotient hook -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 1024, 2048])
def test_quotient_values_equal_the_oracle(n):
    eng = K.Engine(0)  # needs no SRS
    try:
        e, a, c = _case(n)
        w = NO.domain_root(NO.log2_exact(n))
        for z, m in [(0x13579BDF + n, None), (0, None)] + [(pow(w, m, R), m) for m in _in_domain(n)]:
            y = e[m] if m is not None else TO.poly_eval(c, z)
            got = K.limbs_to_scalars(eng.quotient_lagrange_limbs(a, K.Scalar(z), K.Scalar(y)))
            assert got == LO.quotient_evals(e, z, y), (z, m)
            with pytest.raises(K.KzgError) as ei:
                eng.quotient_lagrange_limbs(a, K.Scalar(z), K.Scalar(y + 1))
            assert ei.value.status == K.KZG_ERR_REMAINDER
        const = K.scalars_to_limbs([9] * n)
        assert K.limbs_to_scalars(eng.quotient_lagrange_limbs(const, K.Scalar(3), K.Scalar(9))) == [0] * n
        with pytest.raises(K.KzgError) as ei:
            eng.quotient_lagrange_limbs(const, K.Scalar(3), K.Scalar(8))
        assert ei.value.status == K.KZG_ERR_CONSTANT_POLY
    finally:
        eng.close()


# ---- a basis given as bytes ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def given(engines):
    """the basis of the bench setup at n = 1024 as it would travel: (first context, compressed points, their values' commitment)"""
    eng = engines.bench_srs(1024)
    eng.lagrange_prepare(10)
    pts = _compress_rows(eng.lagrange_read(0, 1024))
    a = _case(1024)[1]
    return eng, pts, eng.commit_lagrange_limbs(a).compress()


def _ordered(pts, order):
    return b"".join(LO.bit_reverse(pts) if order == K.KZG_ORDER_BIT_REVERSED else pts)


@pytest.fixture()
def fresh():
    eng = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(1024)
    yield eng
    eng.close()


@pytest.mark.parametrize("order", [K.KZG_ORDER_NATURAL, K.KZG_ORDER_BIT_REVERSED])
def test_given_basis_is_checked_and_adopted(given, fresh, order):
    first, pts, commitment = given
    a = _case(1024)[1]
    swapped = list(pts)
    swapped[5], swapped[700] = swapped[700], swapped[5]
    assert fresh.lagrange_load_compressed(_ordered(swapped, order), order) is False  # consistent == 0: not adopted
    assert fresh.lagrange_len() == 0
    assert fresh.lagrange_load_compressed(_ordered(pts, order), order) is True
    assert fresh.lagrange_len() == 1024
    assert _compress_rows(fresh.lagrange_read(0, 1024)) == pts
    assert fresh.commit_lagrange_limbs(a).compress() == commitment
    assert fresh.lagrange_load_compressed(_ordered(swapped, order), order) is False  # ... and the held basis stays
    assert fresh.commit_lagrange_limbs(a).compress() == commitment
    assert fresh.lagrange_load_compressed(_ordered(swapped, order), order, check=False) is True  # unchecked: adopted as given
    assert fresh.commit_lagrange_limbs(a).compress() != commitment


@pytest.mark.parametrize("order", [K.KZG_ORDER_NATURAL, K.KZG_ORDER_BIT_REVERSED])
def test_given_basis_with_a_bad_point_is_refused(given, fresh, order):
    first, pts, _ = given
    tp = TO.torsion_points()[11]
    at = 301
    wire = LO.bit_reverse(pts) if order == K.KZG_ORDER_BIT_REVERSED else list(pts)
    shifted = T.g1_compress(T.g1_add(T.g1_uncompress(wire[at]), tp))  # on the curve, outside G1
    for bad, what in ((OFF_CURVE48, "compressed point"), (shifted, "not in G1")):
        data = b"".join(wire[:at] + [bad] + wire[at + 1:])
        for load in (lambda: fresh.lagrange_load_compressed(data, order), lambda: K.Engine(0).srs_load_lagrange_compressed(data, order)):
            with pytest.raises(K.KzgError) as ei:
                load()
            assert ei.value.status == K.KZG_ERR_INVALID_ARG and ei.value.bad_index == at, (what, ei.value)
            assert what in str(ei.value)
        assert fresh.lagrange_len() == 0


@pytest.mark.parametrize("order", [K.KZG_ORDER_NATURAL, K.KZG_ORDER_BIT_REVERSED])
def test_setup_from_its_lagrange_form_alone(given, order):
    first, pts, commitment = given
    a = _case(1024)[1]
    eng = K.Engine(0)
    try:
        eng.srs_load_lagrange_compressed(_ordered(pts, order), order)
        assert eng.srs_len() == 1024 and eng.lagrange_len() == 1024
        assert np.array_equal(eng.srs_read(0, 1024), first.srs_read(0, 1024))  # the monomial SRS, bit for bit
        assert eng.commit_limbs(a).compress() == first.commit_limbs(a).compress()
        assert eng.commit_lagrange_limbs(a).compress() == commitment
    finally:
        eng.close()


# ---- lifetime ----------------------------------------------------------------------------------------------------------------
def test_the_basis_goes_with_the_srs(oracle):
    n, k = 64, 6
    e = _evals(n, 64)
    a = K.scalars_to_limbs(e)
    eng = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(n)
    try:
        assert eng.lagrange_len() == 0
        assert eng.commit_lagrange_limbs(a).compress() == TO.g1_scalar(oracle, NO.barycentric_eval(e, S))
        assert eng.lagrange_len() == n
        s2 = 0x1F2E3D4C5B6A7988
        eng.srs_generate(TO.secret_be(s2), n)
        assert eng.lagrange_len() == 0  # dropped, not rebuilt
        assert eng.commit_lagrange_limbs(a).compress() == TO.g1_scalar(oracle, NO.barycentric_eval(e, s2))
        assert eng.lagrange_len() == n
        tau = 0x77665544332211
        eng.srs_update(TO.secret_be(tau))
        assert eng.lagrange_len() == 0
        assert eng.commit_lagrange_limbs(a).compress() == TO.g1_scalar(oracle, NO.barycentric_eval(e, s2 * tau))
        assert _compress_rows(eng.lagrange_read(0, n)) == _expected_basis(oracle, k, s2 * tau % R)
        eng.lagrange_prepare(5)  # another size replaces the basis
        assert eng.lagrange_len() == 32
        assert _compress_rows(eng.lagrange_read(0, 32)) == _expected_basis(oracle, 5, s2 * tau % R)
        assert eng.commit_lagrange_limbs(a).compress() == TO.g1_scalar(oracle, NO.barycentric_eval(e, s2 * tau))
        assert eng.lagrange_len() == n
    finally:
        eng.close()


# ---- multi-device contexts ---------------------------------------------------------------------------------------------------
def test_multi_device_contexts(oracle):
    n = 2048
    e, a, c = _case(n)
    z = pow(NO.domain_root(11), 1024, R)
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(T.BENCH_SECRET_BE, n)
        assert rep.commit_lagrange_limbs(a).compress() == TO.g1_scalar(oracle, NO.barycentric_eval(e, S))
        assert rep.lagrange_len() == n
        assert rep.open_lagrange_limbs(a, K.Scalar(z), K.Scalar(e[1024])).compress() == TO.proof(oracle, c, z, S, e[1024])
        assert [p.compress() for p in rep.commit_lagrange_batch([a, a])] == [rep.commit_lagrange_limbs(a).compress()] * 2
        assert _compress_rows(rep.lagrange_read(7, 1)) == [TO.g1_scalar(oracle, LO.lagrange_at(11, S)[7])]
        assert K.limbs_to_scalars(rep.quotient_lagrange_limbs(a, K.Scalar(z), K.Scalar(e[1024]))) == LO.quotient_evals(e, z, e[1024])
    finally:
        rep.close()
    rng = K.Engine(devices=[0, 0])
    try:
        rng.srs_generate(T.BENCH_SECRET_BE, n)
        lib = K.load_library()
        for call in (lambda: rng.commit_lagrange_limbs(a), lambda: rng.open_lagrange_limbs(a, K.Scalar(5), K.Scalar(1)),
                     lambda: rng.lagrange_prepare(11), lambda: rng.commit_lagrange_batch([a])):
            with pytest.raises(K.KzgError) as ei:
                call()
            assert ei.value.status == K.KZG_ERR_INVALID_ARG
            assert b"range-split" in lib.kzg_last_error(rng._h)
        assert rng.lagrange_len() == 0
    finally:
        rng.close()
