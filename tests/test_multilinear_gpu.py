"""GPU: multilinear openings (kzg_ml_fold .. kzg_ml_open) against the big-integer restatement
(tests/multilinear_oracle.py), [v]G of the trapdoor oracle, kzg_commit of every level and kzg_open_sets of the padded stack, bit for
bit.  The values are made and compared as blst_fr images: folds, values and F are linear in them, so the oracle works on the images
directly; only the scalar of a group element takes the factor 2^256 out."""
import functools

import numpy as np
import pytest

import bigint_twin as T
import device_arena as DA
import kzg_poly_commit_exploration_amd as K
import multilinear_oracle as MO
import open_combined_oracle as CO
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu
R = K.R_MODULUS
RINV = CO.RINV
BENCH_S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)
# in-lane only (1, 2, 3), in-wave (4, 9), the LDS levels (10), exactly one tile (11), the second launch with 2 and 4 values
# (12, 13), 32 tiles (16)
FOLD_ELLS = (1, 2, 3, 4, 9, 10, 11, 12, 13, 16)
DEVICE_ELLS = (3, 11, 13, 16)
OPEN_ELLS = (1, 2, 3, 5, 12, 16)


def _scalars(vals):
    return [K.Scalar(v) for v in vals]


@functools.lru_cache(maxsize=None)
def _case(ell, kind, ukind, seed=0):
    """(images (n, 4), the same as integers, u, the levels f_1 .. f_l as integers): computed once, shared, never modified"""
    n = 1 << ell
    a = MO.family(kind, n, seed + ell)
    a.setflags(write=False)
    f = CO.images_from_limbs(a)
    u = MO.point_u(ell, ukind, seed + ell)
    return a, f, u, MO.folds(f, u)


def _flat(levels):
    return [c for lv in levels for c in lv]


@pytest.fixture(scope="module")
def eng():
    e = K.Engine(0)
    yield e
    e.close()


def _fold_cases(ell):
    out = [(kind, "random") for kind in MO.FAMILIES] + [("random", k) for k in range(4)] + [("max", k) for k in range(4)]
    return out if ell <= 13 else out[:7] + out[7:11]


@pytest.mark.parametrize("ell", FOLD_ELLS)
def test_fold_and_evaluate(eng, ell):
    """every level of the pyramid element-wise, and v, for every family of values and u with 0, 1, r - 1, 1/2 at every level"""
    for kind, ukind in _fold_cases(ell):
        a, f, u, levels = _case(ell, kind, ukind)
        got = eng.ml_fold(a, _scalars(u))
        want = CO.limbs_from_images(_flat(levels))
        assert got.shape == want.shape == ((1 << ell) - 1, 4)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (kind, ukind, "first differing pyramid index", int(bad[0]), bad.size)
        v = eng.ml_evaluate(a, _scalars(u))
        assert v.v == levels[-1][0] * RINV % R, (kind, ukind)
        if ell <= 10 and kind == "random":
            assert levels[-1][0] == MO.hypercube_eval(f, u)
        if kind == "pairs":  # every u_0 gives the evens
            assert levels[0] == f[0::2]


class _Resident:
    """the values of a case and a pyramid buffer on the device"""

    def __init__(self, e, a):
        self.e, n = e, a.shape[0]
        self.d_evals, self.d_pyr = e.dev_alloc(32 * n), e.dev_alloc(32 * n)
        e.dev_upload(self.d_evals, a)

    def close(self):
        self.e.dev_free(self.d_evals)
        self.e.dev_free(self.d_pyr)


def _g1(oracle, scalar):
    return TO.g1_scalar(oracle, scalar)


@pytest.mark.parametrize("ell", DEVICE_ELLS)
def test_commit_folds(engines, oracle, ell):
    """each C_i is kzg_commit of that level and [f_i(s)]G; the second case has every level zero (infinity)"""
    e = engines.bench_srs(1 << ell)
    for kind, ukind in (("random", "random"), ("zero_levels", 0)):
        if kind == "zero_levels":  # the evens are zero and u_0 = 0: f_1 = 0, and so is every later level
            a = MO.random_images(1 << ell, 77).copy()
            a[0::2] = 0
            f, u = CO.images_from_limbs(a), MO.point_u(ell, 0)
            levels = MO.folds(f, u)
            assert not any(levels[0])
        else:
            a, f, u, levels = _case(ell, kind, ukind)
        res = _Resident(e, a)
        try:
            v = e.ml_fold_device(res.d_evals, ell, _scalars(u), res.d_pyr)
            assert v.v == levels[-1][0] * RINV % R
            got = e.ml_commit_folds_device(res.d_pyr, ell)
        finally:
            res.close()
        assert len(got) == ell - 1
        for i, c in enumerate(got):
            lv = levels[i]
            assert c == e.commit_limbs(CO.limbs_from_images(lv)), (kind, "level", i + 1)
            assert c.compress() == _g1(oracle, TO.commitment_scalar([x * RINV % R for x in lv], BENCH_S)), (kind, "level", i + 1)
            if kind == "zero_levels":
                assert c.is_infinity()


@pytest.mark.parametrize("ell", DEVICE_ELLS)
def test_evaluations_device(eng, ell):
    """the 3 l values for a random r, a small one and r - 2"""
    a, f, u, levels = _case(ell, "random", "random")
    res = _Resident(eng, a)
    try:
        eng.ml_fold_device(res.d_evals, ell, _scalars(u), res.d_pyr)
        for r in (MO.random_scalar(900 + ell), 2, R - 2):
            got = eng.ml_evaluations_device(res.d_evals, res.d_pyr, ell, K.Scalar(r))
            want = MO.values(f, u, r)
            assert [[y.v for y in row] for row in got] == [[y * RINV % R for y in row] for row in want], r
    finally:
        res.close()


@pytest.mark.parametrize("ell", OPEN_ELLS)
def test_open(engines, oracle, ell):
    """kzg_ml_open: W and the values are kzg_open_sets of the padded stack bit for bit, W is the trapdoor's [h(s)]G, kzg_ml_verify
    accepts the proof and rejects it with one value changed, and the chain of the four device forms gives the same bytes"""
    n = 1 << ell
    e = engines.bench_srs(max(n, 4))
    a, f, u, levels = _case(ell, "random", "random", 3)
    r, gamma = MO.random_scalar(40 + ell), MO.random_scalar(80 + ell)
    v, folds, ys, w = e.ml_open(a, _scalars(u), K.Scalar(r), K.Scalar(gamma))
    assert v.v == levels[-1][0] * RINV % R
    # the existing call on the padded stack: t = l polynomials, one set
    stack = np.zeros((ell, n, 4), dtype=np.uint64)
    for i, p in enumerate(MO.padded_stack(f, u)):
        stack[i] = CO.limbs_from_images(p)
    sets = [_scalars(MO.points(r))]
    ys_sets, w_sets = e.open_sets_limbs(stack, [0] * ell, sets, K.Scalar(gamma))
    assert w == w_sets and w.compress() == w_sets.compress()
    assert [[y.v for y in row] for row in ys] == [[y.v for y in row] for row in ys_sets]
    assert [[y.v for y in row] for row in ys] == [[y * RINV % R for y in row] for row in MO.values(f, u, r)]
    plain = [x * RINV % R for x in f]
    assert w.compress() == _g1(oracle, MO.proof_scalar(plain, u, r, gamma, BENCH_S))
    if ell == 1:
        assert w.is_infinity() and folds == []
    for c, sc in zip(folds, MO.fold_commitment_scalars(plain, u, BENCH_S)):
        assert c.compress() == _g1(oracle, sc)
    # the verifier
    com = e.commit_limbs(a)
    g1 = e.srs_read(0, 3)
    g2 = np.stack([K.srs_g2_at(T.BENCH_SECRET_BE, j) for j in range(4)])
    su, sr, sg = _scalars(u), K.Scalar(r), K.Scalar(gamma)
    assert K.ml_verify(com, su, v, folds, ys, sr, sg, w, g1, g2)
    bad = [list(row) for row in ys]
    bad[ell - 1][ell % 3] = K.Scalar((bad[ell - 1][ell % 3].v + 1) % R)
    assert not K.ml_verify(com, su, v, folds, bad, sr, sg, w, g1, g2)
    # the four rounds over caller-held buffers
    res = _Resident(e, a)
    try:
        v2 = e.ml_fold_device(res.d_evals, ell, su, res.d_pyr)
        folds2 = e.ml_commit_folds_device(res.d_pyr, ell)
        ys2 = e.ml_evaluations_device(res.d_evals, res.d_pyr, ell, sr)
        w2 = e.ml_open_device(res.d_evals, res.d_pyr, ell, sr, sg)
    finally:
        res.close()
    assert v2.v == v.v and folds2 == folds and w2 == w
    assert [[y.v for y in row] for row in ys2] == [[y.v for y in row] for row in ys]


@pytest.mark.parametrize("ell", (3, 12))
def test_device_forms_write_only_their_outputs(engines, ell):
    """inside guard bands: the fold writes the declared n - 1 pyramid values and nothing else, the other rounds write nothing"""
    n = 1 << ell
    e = engines.bench_srs(max(n, 4))
    a, f, u, levels = _case(ell, "random", "random")
    with DA.Arena(e, seed=ell) as arena:
        r_in = arena.region(n, name="evals", data=a)
        r_pyr = arena.region(n - 1, name="pyramid")
        arena.upload()
        e.ml_fold_device(r_in.ptr, ell, _scalars(u), r_pyr.ptr)
        want = CO.limbs_from_images(_flat(levels))
        arena.check({r_pyr: want})
        e.ml_commit_folds_device(r_pyr.ptr, ell)
        e.ml_evaluations_device(r_in.ptr, r_pyr.ptr, ell, K.Scalar(5))
        e.ml_open_device(r_in.ptr, r_pyr.ptr, ell, K.Scalar(5), K.Scalar(7))
        arena.check({r_pyr: want})


def test_workspace_reuse(engines):
    """l = 16, then 3, then 16 on one context: the slot's buffers are grown, kept and reused, the bytes are the same"""
    e = engines.bench_srs(1 << 16)
    outs = []
    for ell in (16, 3, 16):
        a, f, u, levels = _case(ell, "random", "random", 3)
        v, folds, ys, w = e.ml_open(a, _scalars(u), K.Scalar(11), K.Scalar(13))
        outs.append((v.v, [c.compress() for c in folds], [[y.v for y in row] for row in ys], w.compress()))
        assert v.v == levels[-1][0] * RINV % R
    assert outs[0] == outs[2]


def test_argument_errors_leave_outputs_unwritten(engines):
    e = engines.bench_srs(16)
    ell = 3
    a, f, u, levels = _case(ell, "random", "random")
    lib, h = e._lib, e._h
    us = np.stack([K.Scalar(x).limbs() for x in u]).astype(np.uint64)
    big = CO.limbs_from_images([R])[0].copy()  # not below r
    fill = np.uint64(0xA5A5A5A5A5A5A5A5)
    v, folds, ys, w = (np.full(4, fill), np.full((ell - 1, 18), fill), np.full((3 * ell, 4), fill), np.full(18, fill))
    pyr = np.full(((1 << ell) - 1, 4), fill)
    good_r, good_g = K.Scalar(5).limbs(), K.Scalar(7).limbs()

    def p(x):
        return x.ctypes.data

    def call(ell_=ell, us_=us, r_=good_r, g_=good_g):
        return lib.kzg_ml_open(h, p(a), ell_, p(us_), p(r_), p(g_), p(v), p(folds), p(ys), p(w))

    bad_us = us.copy()
    bad_us[1] = big
    for r_bad in (0, 1, R - 1):
        assert call(r_=K.Scalar(r_bad).limbs()) == K.KZG_ERR_INVALID_ARG
    assert call(r_=big) == K.KZG_ERR_INVALID_ARG
    assert call(g_=big) == K.KZG_ERR_INVALID_ARG
    assert call(us_=bad_us) == K.KZG_ERR_INVALID_ARG
    assert call(ell_=0) == K.KZG_ERR_INVALID_ARG
    assert call(ell_=K.KZG_ML_MAX_VARS + 1) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_ml_open(h, None, ell, p(us), p(good_r), p(good_g), p(v), p(folds), p(ys), p(w)) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_ml_open(h, p(a), ell, p(us), p(good_r), p(good_g), p(v), p(folds), p(ys), None) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_ml_fold(h, p(a), ell, p(bad_us), p(pyr)) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_ml_fold(h, p(a), 0, p(us), p(pyr)) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_ml_evaluate(h, p(a), ell, p(bad_us), p(v)) == K.KZG_ERR_INVALID_ARG
    for out in (v, folds, ys, w, pyr):
        assert (out == fill).all()
    # a quotient longer than the SRS: kzg_open_points' degree error, and again nothing is written
    small = engines.bench_srs(4)
    a5, f5, u5, _ = _case(5, "random", "random")
    us5 = np.stack([K.Scalar(x).limbs() for x in u5]).astype(np.uint64)
    folds5, ys5 = np.full((4, 18), fill), np.full((15, 4), fill)
    rc = small._lib.kzg_ml_open(small._h, p(a5), 5, p(us5), p(good_r), p(good_g), p(v), p(folds5), p(ys5), p(w))
    assert rc == K.KZG_ERR_DEGREE_TOO_HIGH
    for out in (v, folds5, ys5, w):
        assert (out == fill).all()
    assert call() == K.KZG_OK and not (w == fill).all()
