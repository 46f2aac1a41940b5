"""CPU: tests/multilinear_oracle.py against itself, and kzg_ml_verify (host only) on proofs the oracle builds under a known secret:
the points are [scalar]G from the C oracle, so no device takes part."""
import ctypes

import numpy as np
import pytest

import kzg_poly_commit_exploration_amd as K
import multilinear_oracle as MO
import open_sets_oracle as SO
import trapdoor_oracle as TO

R = MO.R
SECRET = 0x1F2E3D4C5B6A79880123456789ABCDEFFEDCBA98765432100F1E2D3C4B5A6978 % R
ELLS = (1, 2, 3, 6)


def _values(ell, seed):
    rng = np.random.default_rng(seed)
    return [int(x) * 0x9E3779B97F4A7C15F39CC0605CEDC835 % R for x in rng.integers(1, 1 << 62, size=1 << ell)]


# ---- the oracle against itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", (1, 2, 3, 6, 10))
def test_folds_end_in_the_hypercube_sum(ell):
    f = _values(ell, ell)
    for u in (MO.point_u(ell, "random", 5), MO.point_u(ell, 0), MO.point_u(ell, 1), MO.point_u(ell, 2), MO.point_u(ell, 3)):
        levels = MO.folds(f, u)
        assert [len(lv) for lv in levels] == [1 << (ell - 1 - i) for i in range(ell)]
        assert levels[-1][0] == MO.hypercube_eval(f, u)
        assert MO.pyramid(f, u)[MO.level_offset(1 << ell, ell)] == levels[-1][0]


def test_a_vertex_of_the_cube_gives_the_value():
    f = _values(4, 1)
    for j in range(16):
        assert MO.hypercube_eval(f, [(j >> i) & 1 for i in range(4)]) == f[j]


@pytest.mark.parametrize("ell", ELLS)
def test_star_holds_for_honest_values_and_for_no_others(ell):
    f, u, r = _values(ell, 10 + ell), MO.point_u(ell, "random", 7), MO.random_scalar(99)
    v, ys = MO.folds(f, u)[-1][0], MO.values(f, u, r)
    assert MO.star_holds(u, v, ys, r)
    assert not MO.star_holds(u, (v + 1) % R, ys, r)
    for i in range(ell):
        for p in range(3):
            bad = [list(row) for row in ys]
            bad[i][p] = (bad[i][p] + 1) % R
            if p == 2 and i == 0:
                continue  # f_0(r^2) enters no relation: only the opening binds it
            assert not MO.star_holds(u, v, bad, r), (i, p)


@pytest.mark.parametrize("ell", ELLS)
def test_proof_scalar_is_the_set_opening_of_the_padded_stack(ell):
    f, u = _values(ell, 20 + ell), MO.point_u(ell, "random", 8)
    r, gamma = MO.random_scalar(31), MO.random_scalar(32)
    stack = MO.padded_stack(f, u)
    want = SO.proof_scalar(stack, [0] * ell, [MO.points(r)], gamma, SECRET)
    assert MO.proof_scalar(f, u, r, gamma, SECRET) == want
    assert SO.values(stack, [0] * ell, [MO.points(r)]) == MO.values(f, u, r)


# ---- kzg_ml_verify ---------------------------------------------------------------------------------------------------------------
def _point(oracle, v):
    return K.G1Point(oracle.p1_mult(oracle.p1_generator(), v % R))


@pytest.fixture(scope="module")
def setup(oracle):
    g1 = np.stack([oracle.p1_mult(oracle.p1_generator(), pow(SECRET, j, R)) for j in range(3)])
    g2 = np.stack([K.srs_g2_at(TO.secret_be(SECRET), j) for j in range(4)])
    return g1, g2


class Proof:
    def __init__(self, oracle, ell, seed=0):
        self.ell = ell
        self.f, self.u = _values(ell, 40 + ell + seed), MO.point_u(ell, "random", 9 + seed)
        self.r, self.gamma = MO.random_scalar(50 + seed), MO.random_scalar(60 + seed)
        self.v = MO.folds(self.f, self.u)[-1][0]
        self.ys = MO.values(self.f, self.u, self.r)
        self.com = _point(oracle, TO.commitment_scalar(self.f, SECRET))
        self.folds = [_point(oracle, s) for s in MO.fold_commitment_scalars(self.f, self.u, SECRET)]
        self.w = _point(oracle, MO.proof_scalar(self.f, self.u, self.r, self.gamma, SECRET))

    def verify(self, setup, **change):
        g = lambda name: change.get(name, getattr(self, name))
        sc = lambda vals: [K.Scalar(x) for x in vals]
        return K.ml_verify(g("com"), sc(g("u")), K.Scalar(g("v")), g("folds"), [sc(row) for row in g("ys")], K.Scalar(g("r")),
                           K.Scalar(g("gamma")), g("w"), setup[0], setup[1], ell=change.get("ell"))


@pytest.mark.parametrize("ell", ELLS)
def test_verify_accepts_the_honest_proof_and_no_single_change(oracle, setup, ell):
    p = Proof(oracle, ell)
    assert p.verify(setup)
    assert not p.verify(setup, v=(p.v + 1) % R)
    for i in range(ell):
        for k in range(3):
            bad = [list(row) for row in p.ys]
            bad[i][k] = (bad[i][k] + 1) % R
            assert not p.verify(setup, ys=bad), (i, k)
        bad_u = list(p.u)
        bad_u[i] = (bad_u[i] + 1) % R
        assert not p.verify(setup, u=bad_u), i
    other = _point(oracle, 12345)
    for i in range(ell - 1):
        bad = list(p.folds)
        bad[i] = other
        assert not p.verify(setup, folds=bad), i
    assert not p.verify(setup, com=other)
    assert not p.verify(setup, r=(p.r + 1) % R)
    # gamma weighs f_1 .. f_(l-1).  For l <= 2 they have at most two coefficients, so each equals its interpolant on the three
    # points and its term of the check vanishes identically: every gamma verifies, and rightly so.  From l = 3 on it binds.
    assert p.verify(setup, gamma=(p.gamma + 1) % R) == (ell <= 2)
    assert not p.verify(setup, w=other)
    if ell == 1:
        assert p.w.is_infinity() and p.folds == []


@pytest.mark.parametrize("ell", (2, 3, 6))
def test_verify_rejects_a_proof_presented_with_another_ell(oracle, setup, ell):
    p = Proof(oracle, ell, seed=1)
    # one level fewer: the last fold commitment, its values and the last coordinate dropped
    assert not p.verify(setup, ell=ell - 1, u=p.u[:-1], folds=p.folds[:-1], ys=p.ys[:-1])
    # one level more: an extra coordinate, the last level's commitment and values repeated
    extra = p.folds[-1] if p.folds else p.com
    assert not p.verify(setup, ell=ell + 1, u=p.u + [5], folds=p.folds + [extra], ys=p.ys + [p.ys[-1]])


def test_verify_argument_errors(oracle, setup):
    """in the documented order: NULL, l out of range, a scalar not below r, r in {0, 1, r - 1}"""
    ell = 3
    p = Proof(oracle, ell, seed=2)
    lib = K.load_library()
    g1, g2 = (np.ascontiguousarray(x, dtype=np.uint64) for x in setup)
    rows = lambda vals: np.ascontiguousarray(np.stack([K.Scalar(x).limbs() for x in vals]), dtype=np.uint64)
    big = np.frombuffer(int(R).to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
    args = {"com": np.ascontiguousarray(p.com.p1, dtype=np.uint64), "us": rows(p.u), "v": rows([p.v]),
            "folds": np.ascontiguousarray(np.stack([c.p1 for c in p.folds]), dtype=np.uint64),
            "ys": rows([y for row in p.ys for y in row]), "r": rows([p.r]), "gamma": rows([p.gamma]),
            "w": np.ascontiguousarray(p.w.p1, dtype=np.uint64)}

    def call(ell_=ell, **change):
        a = {k: change.get(k, v) for k, v in args.items()}
        ptr = lambda x: None if x is None else x.ctypes.data
        ok = ctypes.c_int(-7)
        rc = lib.kzg_ml_verify(ptr(a["com"]), ell_, ptr(a["us"]), ptr(a["v"]), ptr(a["folds"]), ptr(a["ys"]), ptr(a["r"]),
                               ptr(a["gamma"]), ptr(a["w"]), g1.ctypes.data, 144, g2.ctypes.data, 288, ctypes.byref(ok))
        return rc, ok.value

    assert call() == (K.KZG_OK, 1)
    for name in args:
        assert call(**{name: None}) == (K.KZG_ERR_INVALID_ARG, -7), name
    assert call(0) == (K.KZG_ERR_INVALID_ARG, -7) and call(K.KZG_ML_MAX_VARS + 1) == (K.KZG_ERR_INVALID_ARG, -7)
    bad_us, bad_ys = args["us"].copy(), args["ys"].copy()
    bad_us[2], bad_ys[4] = big, big
    for change in ({"us": bad_us}, {"ys": bad_ys}, {"v": big.reshape(1, 4)}, {"r": big.reshape(1, 4)}, {"gamma": big.reshape(1, 4)}):
        assert call(**change) == (K.KZG_ERR_INVALID_ARG, -7), list(change)
    for r in (0, 1, R - 1):
        assert call(r=rows([r])) == (K.KZG_ERR_INVALID_ARG, -7), r
    off_curve = args["w"].copy()
    off_curve[0] ^= np.uint64(1)
    assert call(w=off_curve) == (K.KZG_ERR_INVALID_ARG, -7)
    # a failing relation is an answer, not an error
    assert call(v=rows([(p.v + 1) % R])) == (K.KZG_OK, 0)
