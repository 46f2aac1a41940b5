"""CPU: the host side of the openings at several point sets -- kzg_verify_sets on trapdoor-made inputs
(commitments [P_i(s)]G and the proof [h(s)]G from the known secret), its agreement with kzg_verify_points, kzg_verify_combined
and the pairing twin, the argument errors, and the export of every new symbol."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import bigint_twin as T
import kzg_poly_commit_exploration_amd as K
import open_sets_oracle as SO
import pairing_twin as PT
import trapdoor_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = K.R_MODULUS
NEW_SYMBOLS = ("kzg_open_sets", "kzg_open_sets_submit", "kzg_wait_sets", "kzg_quotient_sets", "kzg_verify_sets")
SECRET = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % R
N = 9


def _point(oracle, v):
    return K.G1Point(oracle.p1_mult(oracle.p1_generator(), v % R))


@pytest.fixture(scope="module")
def srs(oracle):
    """[s^j]G1 for j < 16 and [s^j]G2 for j <= 16"""
    g1 = np.stack([oracle.p1_mult(oracle.p1_generator(), pow(SECRET, j, R)) for j in range(16)])
    g2 = np.stack([K.srs_g2_at(TO.secret_be(SECRET), j) for j in range(17)])
    return g1, g2


def _points(rng):
    """sixteen distinct points: z, z w (w the 8th root of unity), then random ones"""
    z = rng.randrange(1, R)
    pts = [z, z * SO.ROOT8 % R]
    while len(pts) < 16:
        p = rng.randrange(R)
        if p not in pts:
            pts.append(p)
    return pts


def _case(oracle, name, seed, n=N):
    rng = random.Random(seed)
    t, set_of, sets = SO.shape(name, _points(rng))
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(t)]
    gamma = rng.randrange(R)
    scalars = [TO.poly_eval(p, SECRET) for p in polys]
    return dict(t=t, set_of=set_of, sets=sets, polys=polys, gamma=gamma, scalars=scalars, ys=SO.values(polys, set_of, sets),
                w=SO.proof_scalar(polys, set_of, sets, gamma, SECRET), commitments=[_point(oracle, c) for c in scalars])


def _verify(d, srs, oracle, **changes):
    d = dict(d, **changes)
    proof = d.get("proof") or _point(oracle, d["w"])
    return K.verify_sets(d["commitments"], d["set_of"], [[K.Scalar(z) for z in s] for s in d["sets"]],
                         [[K.Scalar(y) for y in row] for row in d["ys"]], K.Scalar(d["gamma"]), proof, srs[0], srs[1])


def test_abi_exports_the_new_symbols():
    lib = K.load_library()
    header = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in K.ABI_SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, header), name
    assert "#define KZG_MAX_SETS 8" in header and K.KZG_MAX_SETS == 8
    assert "#define KZG_MAX_SET_POINTS 16" in header and K.KZG_MAX_SET_POINTS == 16
    for name in ("open_sets_limbs", "open_sets_submit", "wait_sets", "quotient_sets_limbs"):
        assert callable(getattr(K.Engine, name)), name
    assert callable(K.verify_sets) and "verify_sets" in K.__all__
    assert "KZG_MAX_SETS" in K.__all__ and "KZG_MAX_SET_POINTS" in K.__all__
    # the header says what gamma has to be, and that nothing is hashed here
    section = header[header.index("openings at several point sets"):header.index("#define KZG_MAX_SETS")]
    assert "AFTER the commitments and the values" in section and "Nothing is hashed here" in section


@pytest.mark.parametrize("name", sorted(SO.SHAPES))
def test_verify_sets_accepts_and_rejects(oracle, srs, name):
    d = _case(oracle, name, 100 + sorted(SO.SHAPES).index(name))
    t, set_of, sets = d["t"], d["set_of"], d["sets"]
    assert _verify(d, srs, oracle)
    # one value changed
    for i in sorted({0, t // 2, t - 1}):
        ys = [list(row) for row in d["ys"]]
        ys[i][-1] = (ys[i][-1] + 1) % R
        assert not _verify(d, srs, oracle, ys=ys), i
    # the proof replaced by another point
    assert not _verify(d, srs, oracle, proof=_point(oracle, d["w"] + 1))
    assert not _verify(d, srs, oracle, proof=d["commitments"][0])
    # gamma changed (with one polynomial gamma does not enter)
    assert _verify(d, srs, oracle, gamma=(d["gamma"] + 1) % R) == (t == 1)
    # two set_of entries of different sets swapped (sets of one size: the layout of the values is unchanged)
    swaps = [(i, j) for i in range(t) for j in range(i + 1, t)
             if set_of[i] != set_of[j] and len(sets[set_of[i]]) == len(sets[set_of[j]])]
    if swaps:
        i, j = swaps[0]
        so = list(set_of)
        so[i], so[j] = so[j], so[i]
        assert not _verify(d, srs, oracle, set_of=so)
    # one point changed
    moved = [list(s) for s in sets]
    moved[-1][-1] = (moved[-1][-1] + 1) % R
    assert not _verify(d, srs, oracle, sets=moved)
    # two points of one set swapped without swapping the values
    big = [g for g, s in enumerate(sets) if len(s) >= 2]
    if big:
        swapped = [list(s) for s in sets]
        swapped[big[0]][0], swapped[big[0]][1] = swapped[big[0]][1], swapped[big[0]][0]
        assert not _verify(d, srs, oracle, sets=swapped)
        ys = [list(row) for row in d["ys"]]  # ... and with the values swapped too it is the same statement
        for i in range(t):
            if set_of[i] == big[0]:
                ys[i][0], ys[i][1] = ys[i][1], ys[i][0]
        assert _verify(d, srs, oracle, sets=swapped, ys=ys)


def test_infinity_and_short_polynomials(oracle, srs):
    """n <= min |S_g|: h = 0, the proof is infinity, and the check is the interpolation alone"""
    d = _case(oracle, "eight_pairs", 7, n=2)
    assert d["w"] == 0
    inf = K.G1Point(np.zeros(18, dtype=np.uint64))
    assert _verify(d, srs, oracle, proof=inf)
    ys = [list(row) for row in d["ys"]]
    ys[3][0] = (ys[3][0] + 1) % R
    assert not _verify(d, srs, oracle, proof=inf, ys=ys)


def test_same_verdict_as_verify_points_and_verify_combined(oracle, srs):
    rng = random.Random(5)
    # t = 1, m = 1: a multiproof
    for k in (1, 3, 16):
        zs = _points(rng)[:k]
        p = [rng.randrange(R) for _ in range(N + 8)]
        c = _point(oracle, TO.poly_eval(p, SECRET))
        pi = _point(oracle, TO.multiproof_scalar(p, zs, SECRET))
        ys = [TO.poly_eval(p, z) for z in zs]
        for bad in (None, 0, k - 1):
            yy = [K.Scalar(y + (1 if j == bad else 0)) for j, y in enumerate(ys)]
            a = K.verify_points(c, pi, [K.Scalar(z) for z in zs], yy, srs[0], srs[1])
            b = K.verify_sets([c], [0], [[K.Scalar(z) for z in zs]], [yy], K.Scalar(rng.randrange(R)), pi, srs[0], srs[1])
            assert a == b == (bad is None), (k, bad)
        assert not K.verify_sets([c], [0], [[K.Scalar(z) for z in zs]], [[K.Scalar(y) for y in ys]], K.Scalar(3), c, srs[0], srs[1])
    # |T| = 1: a combined opening
    for t in (1, 2, 17):
        d = _case(oracle, "one_point", 50 + t)
        polys = [[rng.randrange(R) for _ in range(N)] for _ in range(t)]
        z, gamma = d["sets"][0][0], d["gamma"]
        cs = [_point(oracle, TO.poly_eval(p, SECRET)) for p in polys]
        pi = _point(oracle, SO.proof_scalar(polys, [0] * t, [[z]], gamma, SECRET))
        ys = [TO.poly_eval(p, z) for p in polys]
        for bad in (None, 0, t - 1):
            yy = [K.Scalar(y + (1 if i == bad else 0)) for i, y in enumerate(ys)]
            a = K.verify_combined(cs, yy, K.Scalar(z), K.Scalar(gamma), pi, srs[1][1])
            b = K.verify_sets(cs, [0] * t, [[K.Scalar(z)]], [[y] for y in yy], K.Scalar(gamma), pi, srs[0], srs[1])
            assert a == b == (bad is None), (t, bad)


def test_the_equation_through_the_pairing_twin(oracle, srs):
    """the PLONK shape, one valid and one invalid case: prod_g e(A_g, [Z_(T \\ S_g)(s)]G2) == e(W, [Z_T(s)]G2) with the G2
    points made by the twin from the scalars -- without the library's G2 code -- and the library's verdict next to it"""
    d = _case(oracle, "plonk", 77)
    for bad in (False, True):
        ys = [list(row) for row in d["ys"]]
        if bad:
            ys[4][0] = (ys[4][0] + 1) % R
        sides, b_t = SO.verifier_sides(d["scalars"], d["set_of"], d["sets"], ys, d["gamma"], SECRET)
        pairs = [(T.g1_mul(T.G1, a), PT.g2_mul(PT.G2, b)) for a, b in sides]
        pairs.append((T.g1_neg(T.g1_mul(T.G1, d["w"])), PT.g2_mul(PT.G2, b_t)))
        assert PT.pairing_product_is_one(pairs) == (not bad)
        assert _verify(d, srs, oracle, ys=ys) == (not bad)


def test_argument_errors(oracle, srs):
    lib = K.load_library()
    d = _case(oracle, "overlapping", 9)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    u32 = lambda v: np.ascontiguousarray(v, dtype=np.uint32)
    rows = lambda v: np.ascontiguousarray(np.stack([K.Scalar(x).limbs() for x in v]), dtype=np.uint64)
    cs = np.ascontiguousarray(np.stack([c.p1 for c in d["commitments"]]))
    g1, g2 = np.ascontiguousarray(srs[0]), np.ascontiguousarray(srs[1])
    pi = np.ascontiguousarray(_point(oracle, d["w"]).p1)
    ok = ctypes.c_int(0)
    not_fr = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)

    def call(t=d["t"], set_of=d["set_of"], sets=d["sets"], ys=d["ys"], gamma=None, m=None, null=None, zs_rows=None, ys_rows=None,
             commitments=cs, setup_g2=g2):
        zs = zs_rows if zs_rows is not None else rows([z for s in sets for z in s])
        yl = ys_rows if ys_rows is not None else rows([y for row in ys for y in row])
        args = [p(commitments), t, p(u32(set_of)), p(u32([len(s) for s in sets])), len(sets) if m is None else m, p(zs), p(yl),
                p(K.Scalar(d["gamma"]).limbs() if gamma is None else gamma), p(pi), p(g1), 144, p(setup_g2), 288, ctypes.byref(ok)]
        if null is not None:
            args[null] = None
        return lib.kzg_verify_sets(*args)

    bad = K.KZG_ERR_INVALID_ARG
    assert call() == K.KZG_OK and ok.value == 1
    assert call(t=0) == bad and call(t=K.KZG_MAX_COMBINE + 1) == bad
    assert call(m=0) == bad and call(m=K.KZG_MAX_SETS + 1) == bad
    assert call(sets=[d["sets"][0], [], d["sets"][2]]) == bad  # an empty set
    assert call(set_of=[1, 0, 1, 1, 0]) == bad  # a set no polynomial uses
    assert call(set_of=[1, 0, 3, 1, 0]) == bad  # set_of[i] >= m
    a, b, c = d["sets"][1]
    assert call(sets=[d["sets"][0], [a, b, a], d["sets"][2]]) == bad  # two equal points within one set
    for pos in (0, 2, 3, 5, 6, 7, 8, 9, 11, 13):
        assert call(null=pos) == bad, pos
    zs = rows([z for s in d["sets"] for z in s])
    zs[2] = not_fr
    assert call(zs_rows=zs) == bad and call(gamma=not_fr) == bad  # a point or gamma not below r
    yl = rows([y for row in d["ys"] for y in row])
    yl[1] = not_fr
    assert call(ys_rows=yl) == bad
    off_curve, off_twist = cs.copy(), g2.copy()
    off_curve[1, 0] ^= 1
    off_twist[2, 0] ^= 1
    assert call(commitments=off_curve) == bad and call(setup_g2=off_twist) == bad
    # seventeen distinct points are one too many; sixteen over eight sets (m + 1 = 9 pairs) are accepted, nine sets refused
    rng = random.Random(3)
    e = _case(oracle, "eight_pairs", 11)
    assert _verify(e, srs, oracle)
    extra = rng.randrange(R)
    sets17 = [list(s) for s in e["sets"]]
    sets17[7] = sets17[7] + [extra]
    ys17 = [list(row) + ([0] if g == 7 else []) for row, g in zip(e["ys"], e["set_of"])]
    cs8 = np.ascontiguousarray(np.stack([c.p1 for c in e["commitments"]]))
    assert call(t=e["t"], set_of=e["set_of"], sets=sets17, ys=ys17, commitments=cs8) == bad
    nine = [[z] for z in _points(rng)[:9]]
    assert call(t=9, set_of=list(range(9)), sets=nine, ys=[[0]] * 9, commitments=np.zeros((9, 18), dtype=np.uint64)) == bad
    eight = nine[:8]
    assert call(t=8, set_of=list(range(8)), sets=eight, ys=[[0]] * 8, commitments=np.zeros((8, 18), dtype=np.uint64)) == K.KZG_OK
