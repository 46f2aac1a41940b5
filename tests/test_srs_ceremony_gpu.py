"""GPU: a powers-of-tau contribution to the resident SRS (kzg_srs_update) and the verification of a setup (kzg_srs_verify,
kzg_srs_verify_lincomb), DESIGN.md section 4.14.  Every point and every sum is compared, compressed byte for byte, with [v]G1
for the scalar v that the known secrets give (tests/srs_ceremony_oracle.py).  Every test builds its own engine: an update
would poison a shared one.  SRS lengths: 33 crosses the normaliser's batches of 32 points, 65 the wave of 64 lanes."""
import contextlib
import random

import numpy as np
import pytest

import bigint_twin as T
import kzg_poly_commit_exploration_amd as K
import srs_ceremony_oracle as SO
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu
R = K.R_MODULUS
NS = (1, 2, 3, 33, 64, 65, 4097)
S = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543210011223344556677 % R
TAU_RANDOM = 0x5A17C0DE0BADF00D5EEDFACE0123456789ABCDEFFEDCBA98765432100F1E2D3C  # 255 bits
assert TAU_RANDOM.bit_length() == 255 and TAU_RANDOM < R
TAUS = {"one": (1).to_bytes(32, "big"), "two": (2).to_bytes(32, "big"), "r-1": (R - 1).to_bytes(32, "big"),
        "random": TAU_RANDOM.to_bytes(32, "big"), "above_r": b"\xff" * 31 + b"\xfe"}


def _be(v):
    return int(v % R).to_bytes(32, "big")


@contextlib.contextmanager
def _engine(s, n, first=0, **kw):
    e = K.Engine(**kw) if kw else K.Engine(0)
    try:
        e.srs_generate(_be(s), n, first)
        yield e
    finally:
        e.close()


_POINTS = {}


def _point(oracle, v):
    """[v]G1 compressed, one oracle multiplication per distinct scalar"""
    v %= R
    if v not in _POINTS:
        _POINTS[v] = TO.g1_scalar(oracle, v)
    return _POINTS[v]


def _p1(oracle, v):
    return np.asarray(oracle.p1_mult(oracle.p1_generator(), v % R), dtype=np.uint64).reshape(18)


def _compressed(rows):
    return [K.G1Point(r).compress() for r in np.asarray(rows, dtype=np.uint64).reshape(-1, 18)]


def _read(e):
    return e.srs_read(0, e.srs_len())


def _g2(s):
    return np.stack([K.srs_g2_at(_be(s), i) for i in range(2)])


def _assert_srs(e, oracle, scalars, what):
    got = _compressed(_read(e))
    assert len(got) == len(scalars)
    for i, v in enumerate(scalars):
        assert got[i] == _point(oracle, v), (what, i)


# ---- update parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,first,tau", [(65, 0, k) for k in TAUS] + [(33, 1, "random"), (33, (1 << 32) + 5, "random"),
                                                                       (33, (1 << 32) + 5, "r-1"), (3, 1, "above_r")] +
                         [(n, 0, "random") for n in NS if n != 65])
def test_update_equals_the_setup_of_the_product(oracle, n, first, tau):
    tau_v = SO.scalar_of(TAUS[tau])
    with _engine(S, n, first) as e:
        before = _read(e)
        if n <= 65:
            _assert_srs(e, oracle, SO.setup_scalars(S, first, n), "generated")
        e.srs_update(TAUS[tau], first)
        assert e.srs_len() == n
        _assert_srs(e, oracle, SO.updated_scalars(S, [tau_v], first, n), tau)
        if tau == "one":  # bit for bit, not only the same points
            assert np.array_equal(_read(e), before)


def test_chained_updates_equal_one_update_by_the_product(oracle):
    t1, t2, n, first = TAU_RANDOM, (R - 12345), 65, 2
    with _engine(S, n, first) as e:
        e.srs_update(_be(t1), first)
        e.srs_update(_be(t2), first)
        chained = _read(e)
    with _engine(S, n, first) as e:
        e.srs_update(_be(t1 * t2), first)
        assert np.array_equal(_read(e), chained)
        _assert_srs(e, oracle, SO.updated_scalars(S, [t1, t2], first, n), "chained")


@pytest.mark.parametrize("tau", [bytes(32), R.to_bytes(32, "big"), (2 * R).to_bytes(32, "big")])
def test_zero_contribution_is_refused_and_the_srs_kept(oracle, tau):
    with _engine(S, 33) as e:
        before = _read(e)
        with pytest.raises(K.KzgError) as ei:
            e.srs_update(tau)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        assert e.srs_len() == 33 and np.array_equal(_read(e), before)
        c = [3, 1, 4, 1, 5]
        assert e.commit_limbs(K.scalars_to_limbs(c)).compress() == _point(oracle, TO.commitment_scalar(c, S))


def test_update_without_an_srs():
    e = K.Engine(0)
    try:
        with pytest.raises(K.KzgError) as ei:
            e.srs_update(TAUS["two"])
        assert ei.value.status == K.KZG_ERR_NO_SRS
    finally:
        e.close()


def test_infinities_stay_through_an_update(oracle):
    """the setup of secret 0: SRS[0] = G1, every other point infinity"""
    n = 65
    with _engine(0, n) as e:
        e.srs_update(TAUS["random"])
        rows = _read(e)
        assert K.G1Point(rows[0]).compress() == _point(oracle, 1)
        assert all(K.G1Point(r).is_infinity() for r in rows[1:])
        ok, reason, bad = e.srs_verify(_g2(0))
        assert (ok, reason) == (False, K.KZG_SRS_G2_BAD)  # [0]G2 is infinity
        ok, reason, bad = e.srs_verify(_g2(S))
        assert (ok, reason, bad) == (False, K.KZG_SRS_INFINITY, 1)


# ---- everything derived from the SRS follows an update ----------------------------------------------------------------------
def test_commit_and_open_after_an_update(oracle):
    n = 4097
    rnd = random.Random(21)
    st = S * TAU_RANDOM % R
    vals = [rnd.randrange(R) for _ in range(n)]
    limbs = K.scalars_to_limbs(vals)
    z = rnd.randrange(R)
    y = TO.poly_eval(vals, z)
    with _engine(S, n) as e:
        assert e.commit_limbs(limbs).compress() == _point(oracle, TO.commitment_scalar(vals, S))
        e.srs_update(TAUS["random"])
        assert e.commit_limbs(limbs).compress() == _point(oracle, TO.commitment_scalar(vals, st))
        assert e.open_limbs(limbs, K.Scalar(z), K.Scalar(y)).compress() == _point(oracle, TO.proof_scalar(vals, z, st))


def test_fk20_cache_is_dropped_by_an_update(oracle):
    """the transforms of the SRS that kzg_fk20_prepare caches belong to the old secret"""
    n, K_, t = 64, 7, 2
    rnd = random.Random(22)
    st = S * TAU_RANDOM % R
    vals = [rnd.randrange(R) for _ in range(n)]
    c = K.scalars_to_limbs(vals)[None]
    with _engine(S, n) as e:
        e.fk20_prepare(n, t)
        _, proofs = e.cells_and_proofs_fk20(c, K_, t)
        want = TO.cell_proof_scalars_fast(vals, K_, t, S)
        assert [p.compress() for p in proofs[0]] == [_point(oracle, want[j]) for j in range(len(proofs[0]))]
        e.srs_update(TAUS["random"])
        _, proofs = e.cells_and_proofs_fk20(c, K_, t)
        want = TO.cell_proof_scalars_fast(vals, K_, t, st)
        assert [p.compress() for p in proofs[0]] == [_point(oracle, want[j]) for j in range(len(proofs[0]))]


# ---- verification: accepted setups ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_verify_accepts_a_setup_and_follows_an_update(n):
    g2 = _g2(S)
    with _engine(S, n) as e:
        assert e.srs_verify(g2) == (True, K.KZG_SRS_OK, None)
        e.srs_update(TAUS["random"])
        g2_new = np.stack([g2[0], K.g2_mul(g2[1], TAUS["random"])])
        assert np.array_equal(g2_new[1], K.srs_g2_at(_be(S * TAU_RANDOM), 1))
        assert e.srs_verify(g2_new) == (True, K.KZG_SRS_OK, None)
        if n > 1:  # with one point nothing ties G1 to [s]G2
            assert e.srs_verify(g2) == (False, K.KZG_SRS_NOT_POWERS, None)
        else:
            assert e.srs_verify(g2) == (True, K.KZG_SRS_OK, None)


def test_verify_a_slice_with_and_without_the_generator_flag():
    with _engine(S, 33, first=1) as e:
        assert e.srs_verify(_g2(S), require_generator=False) == (True, K.KZG_SRS_OK, None)
        assert e.srs_verify(_g2(S)) == (False, K.KZG_SRS_FIRST_NOT_GENERATOR, 0)


def test_verify_without_an_srs():
    e = K.Engine(0)
    try:
        with pytest.raises(K.KzgError) as ei:
            e.srs_verify(_g2(S))
        assert ei.value.status == K.KZG_ERR_NO_SRS
    finally:
        e.close()


# ---- verification: altered setups, read back, changed on the host and reloaded ---------------------------------------------
@pytest.fixture(scope="module")
def rows65():
    with _engine(S, 65) as e:
        rows = _read(e)
    rows.setflags(write=False)
    return rows


@contextlib.contextmanager
def _loaded(rows):
    e = K.Engine(0)
    try:
        e.srs_load(np.ascontiguousarray(rows))
        yield e
    finally:
        e.close()


@pytest.mark.parametrize("i", [0, 1, 32, 64])
def test_verify_rejects_one_wrong_point(oracle, rows65, i):
    rows = rows65.copy()
    rows[i] = _p1(oracle, pow(S, i, R) + 1)
    with _loaded(rows) as e:
        # index 0 is no longer the generator: without the flag the structure check has to find it
        assert e.srs_verify(_g2(S), require_generator=False) == (False, K.KZG_SRS_NOT_POWERS, None)
        if i == 0:
            assert e.srs_verify(_g2(S)) == (False, K.KZG_SRS_FIRST_NOT_GENERATOR, 0)


def test_verify_rejects_two_swapped_points(rows65):
    rows = rows65.copy()
    rows[[40, 41]] = rows[[41, 40]]
    with _loaded(rows) as e:
        assert e.srs_verify(_g2(S)) == (False, K.KZG_SRS_NOT_POWERS, None)


@pytest.fixture(scope="module")
def torsion():
    return TO.torsion_points()


def _shift(row, tp):
    """the point plus a torsion point, added with kzg_g1_sum"""
    t = np.array(T.g1_to_blst_p1_limbs(tp), dtype=np.uint64)
    return K.G1Point.sum([K.G1Point(row), K.G1Point(t)]).p1


@pytest.mark.parametrize("q", [3, 11])
def test_verify_rejects_points_outside_the_subgroup(rows65, torsion, q):
    """a component of cofactor order pairs to 1: the hook's pairing holds on the shifted setup, only the subgroup check sees it"""
    rnd = random.Random(q)
    for bad in ((64,), (1,), (33, 7)):
        rows = rows65.copy()
        for i in bad:
            rows[i] = _shift(rows[i], torsion[q])
            assert T.g1_is_on_curve(T.g1_from_blst_p1_limbs([int(x) for x in rows[i]]))
        with _loaded(rows) as e:
            assert e.srs_verify(_g2(S)) == (False, K.KZG_SRS_NOT_IN_G1, min(bad))
            weights = [K.Scalar(rnd.randrange(1, R)) for _ in range(64)]
            _, _, valid = e.srs_verify_lincomb(weights, _g2(S))
            assert valid


@pytest.mark.parametrize("k", [1, 33, 64])
def test_verify_rejects_a_point_at_infinity(rows65, torsion, k):
    rows = rows65.copy()
    rows[k] = 0
    rows[0] = _shift(rows[0], torsion[3])  # infinity is reported before a point outside G1, whatever their indices
    with _loaded(rows) as e:
        assert e.srs_verify(_g2(S)) == (False, K.KZG_SRS_INFINITY, k)


def test_verify_g2_inputs(rows65):
    g2 = _g2(S)
    with _loaded(rows65) as e:
        assert e.srs_verify(g2) == (True, K.KZG_SRS_OK, None)
        not_gen = np.stack([K.srs_g2_at(_be(2), 1), g2[1]])
        assert e.srs_verify(not_gen) == (False, K.KZG_SRS_G2_BAD, None)
        inf = np.stack([g2[0], np.zeros(36, dtype=np.uint64)])
        assert e.srs_verify(inf) == (False, K.KZG_SRS_G2_BAD, None)
        off = g2.copy()
        off[1][0] ^= np.uint64(1)  # x moved: not on the twist
        with pytest.raises(K.KzgError) as ei:
            e.srs_verify(off)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        with pytest.raises(K.KzgError) as ei:
            e.srs_verify_lincomb([K.Scalar(1)] * 64, off)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG


# ---- the two sums with given weights ----------------------------------------------------------------------------------------
def _weight_sets(n, scalars, rnd):
    m = n - 1
    sets = {"first": [1] + [0] * (m - 1), "last": [0] * (m - 1) + [1], "ones": [1] * m,
            "random": [rnd.randrange(R) for _ in range(m)],
            "edges": [(0, R - 1, 1, R - 2)[i % 4] for i in range(m)]}
    if m >= 2:  # sum rho_i s^i = 0: A is infinity (and so is B = [s]A)
        w = [rnd.randrange(1, R) for _ in range(m - 1)]
        part = sum(a * b for a, b in zip(w, scalars)) % R
        sets["A=inf"] = w + [-part * pow(scalars[m - 1], R - 2, R) % R]
    return sets


@pytest.mark.parametrize("n,first", [(2, 0), (3, 0), (33, 0), (64, 0), (65, 3), (4097, 0)])
def test_lincomb_sums_against_the_known_secret(oracle, n, first):
    rnd = random.Random(n)
    scalars = SO.setup_scalars(S, first, n)
    g2 = _g2(S)
    with _engine(S, n, first) as e:
        for name, w in _weight_sets(n, scalars, rnd).items():
            a, b, valid = e.srs_verify_lincomb([K.Scalar(v) for v in w], g2)
            want_a, want_b = SO.lincomb_scalars(scalars, w)
            assert a.compress() == _point(oracle, want_a), (name, "A")
            assert b.compress() == _point(oracle, want_b), (name, "B")
            assert valid, name
            if name == "A=inf":
                assert a.is_infinity() and b.is_infinity()
        a, b, valid = e.srs_verify_lincomb([K.Scalar(1)] * (n - 1), _g2(S + 1))
        assert not valid and a.compress() == _point(oracle, sum(scalars[:-1]))


def test_lincomb_of_one_point_and_bad_weights():
    with _engine(S, 1) as e:
        a, b, valid = e.srs_verify_lincomb(np.zeros((0, 4), dtype=np.uint64), _g2(S))
        assert a.is_infinity() and b.is_infinity() and valid
    with _engine(S, 3) as e:
        w = np.stack([K.Scalar(1).limbs(), np.array([2 ** 64 - 1] * 4, dtype=np.uint64)])  # not below r
        with pytest.raises(K.KzgError) as ei:
            e.srs_verify_lincomb(w, _g2(S))
        assert ei.value.status == K.KZG_ERR_INVALID_ARG


# ---- several devices --------------------------------------------------------------------------------------------------------
def test_replicated_context_updates_every_device(oracle):
    n = 65
    st = S * TAU_RANDOM % R
    vals = [7, 0, R - 1, 5] + list(range(1, 62))
    limbs = K.scalars_to_limbs(vals)
    with _engine(S, n, devices=[0, 0, 0], replicate=True) as e:
        e.srs_update(TAUS["random"])
        _assert_srs(e, oracle, SO.updated_scalars(S, [TAU_RANDOM], 0, n), "replicated")
        want = _point(oracle, TO.commitment_scalar(vals, st))
        for _ in range(2 * e.num_devices()):  # the devices take the commitments in turn
            assert e.commit_limbs(limbs).compress() == want
        assert e.srs_verify(np.stack([_g2(S)[0], K.srs_g2_at(_be(st), 1)])) == (True, K.KZG_SRS_OK, None)
        assert e.srs_verify(_g2(S)) == (False, K.KZG_SRS_NOT_POWERS, None)
        with pytest.raises(K.KzgError) as ei:
            e.srs_update(bytes(32))
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        assert e.commit_limbs(limbs).compress() == want


def test_range_split_context_is_refused():
    with _engine(S, 65, devices=[0, 0]) as e:
        before = _read(e)
        with pytest.raises(K.KzgError) as ei:
            e.srs_update(TAUS["two"])
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        with pytest.raises(K.KzgError) as ei:
            e.srs_verify(_g2(S))
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        assert np.array_equal(_read(e), before)
