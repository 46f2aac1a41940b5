"""GPU: the Fr kernels at the magnitudes their "Bounds" comments allow ("Fr magnitudes under test").

The inputs are the families of tests/fr_extremes.py -- half values, digit-extremal images, extremal multipliers, compensated
terms, the NTT chain -- which tests/test_fr_extremes.py shows to fill the lazy sums on the host build of the same headers.
Every comparison is exact, against the big-integer oracles of the other GPU tests.  Coefficients and values are made and
compared as blst_fr images (what the C-ABI carries and what the kernels slice into digits); the operations are linear, so the
oracles work on the images directly and only a point, a weight or a result read as a Scalar has the factor 2^256 taken out."""
import random

import numpy as np
import pytest

import bigint_twin as T
import blob_proof_oracle as BP
import cells_oracle as CL
import fr_extremes as FE
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import open_combined_oracle as CO
import open_points_oracle as PO
import open_sets_oracle as SO
import oracle_ctypes as O
import recover_oracle as RO
import trapdoor_oracle as TO
import verify_cells_oracle as VO
import wire_oracle as W

pytestmark = pytest.mark.gpu
R = FE.R
RINV = CO.RINV
S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)
HALVES = FE.half_values()
MULTS = FE.extremal_multipliers()  # plain values w whose device form w 2^270 mod r is a half value or digit-extremal


def _value(image):
    return image * RINV % R


def _rows(images):
    return CO.limbs_from_images(images)


def _random(seed):
    return random.Random(seed).randrange(2, R)


def _digit_pattern(n, phase=0):
    """n images cycling through D+, D-, the alternating patterns and their tops"""
    fam = FE.digit_extremal()
    return [fam[(j + phase) % len(fam)] for j in range(n)]


@pytest.fixture(scope="module")
def eng():
    e = K.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def srs():
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(4096)
    yield e
    e.close()


# ---- combined openings: k_combine_eval, k_combine_eval_finish --------------------------------------------------------------


def _compensated_block(n, t, gamma, phase):
    """t polynomials of n images with c_i[j] gamma^i = a half value for every i: the 256 products of coefficient j have one
    sign; the half value changes with j so that F is no constant vector"""
    base = [HALVES[(j + phase) % len(HALVES)] for j in range(n)]
    gi = pow(gamma, -1, R)
    polys, x = [], 1
    for _ in range(t):
        polys.append([b * x % R for b in base])
        x = x * gi % R
    return polys


@pytest.mark.parametrize("n", [1, 257, 2049])
def test_combined_openings_sum_256_half_values(eng, n):
    t = 256
    gamma, z = _random(n), _random(n + 1)
    cases = {"H+": ([[FE.H_PLUS] * n] * t, 1), "H-": ([[FE.H_MINUS] * n] * t, 1),
             "compensated": (_compensated_block(n, t, gamma, n), gamma)}
    for name, (polys, g) in cases.items():
        a = np.stack([_rows(p) for p in polys])
        want_f = _rows(CO.combine(polys, g))
        assert np.array_equal(eng.combine_polys_limbs(a, K.Scalar(g)), want_f), name
        if name == "compensated":
            want_y = [_value(y) for y in CO.values(polys, z)]
            assert [y.v for y in eng.evaluate_batch_at_limbs(a, K.Scalar(z), stride=n + 5)] == want_y
            before = eng.max_batch()
            try:  # three passes: F leaves each pass canonical and enters the next as the accumulator's start value
                assert eng.set_max_batch(100) == 100
                assert np.array_equal(eng.combine_polys_limbs(a, K.Scalar(g)), want_f), "three passes"
                assert [y.v for y in eng.evaluate_batch_at_limbs(a, K.Scalar(z))] == want_y, "three passes"
            finally:
                eng.set_max_batch(before)


@pytest.mark.parametrize("n", [1, 257, 2049])
def test_combined_openings_values_of_digit_extremal_coefficients(eng, n):
    polys = [[FE.d_plus(0)] * n, [FE.d_minus(0)] * n, [FE.d_plus(0x73EC)] * n, [FE.d_minus(0x73EC)] * n,
             _digit_pattern(n), _digit_pattern(n, 3)]
    a = np.stack([_rows(p) for p in polys])
    for z in [1] + MULTS:
        want = [_value(y) for y in CO.values(polys, z)]
        assert [y.v for y in eng.evaluate_batch_at_limbs(a, K.Scalar(z))] == want, hex(z)
        assert np.array_equal(eng.combine_polys_limbs(a, K.Scalar(z)), _rows(CO.combine(polys, z))), hex(z)  # z as gamma


# ---- openings at several point sets: k_sets_combine -----------------------------------------------------------------------


def test_sets_256_polynomials_on_one_point(eng):
    n, t = 2049, 256
    gamma, p = _random(11), MULTS[0]
    polys = _compensated_block(n, t, gamma, 0)  # the weight of a set of one point is 1
    a = np.stack([_rows(c) for c in polys])
    set_of, sets = [0] * t, [[p]]
    ys, h = eng.quotient_sets_limbs(a, set_of, [[K.Scalar(p)]], K.Scalar(gamma))
    assert [[y.v for y in row] for row in ys] == [[_value(y) for y in row] for row in SO.values(polys, set_of, sets)]
    assert np.array_equal(h, _rows(SO.quotient(polys, set_of, sets, gamma)))


def test_sets_eight_pairs_compensated(eng):
    """polynomial i on the pair {a, b}: its multiplier is gamma^i / (a - b) at a and the negative at b, so coefficients
    H (a - b) / gamma^i give terms H+ at a and H- at b"""
    n = 2049
    gamma = _random(12)
    points = MULTS + [_random(20 + i) for i in range(10)]
    t, set_of, sets = SO.shape("eight_pairs", points)
    polys = []
    for i in range(t):
        a_, b_ = sets[set_of[i]]
        m = pow(gamma, i, R) * pow(a_ - b_, -1, R) % R
        mi = pow(m, -1, R)
        polys.append([HALVES[(j + i) % len(HALVES)] * mi % R for j in range(n)])
    a = np.stack([_rows(c) for c in polys])
    ys, h = eng.quotient_sets_limbs(a, set_of, [[K.Scalar(z) for z in s] for s in sets], K.Scalar(gamma), stride=n + 5)
    assert [[y.v for y in row] for row in ys] == [[_value(y) for y in row] for row in SO.values(polys, set_of, sets)]
    assert np.array_equal(h, _rows(SO.quotient(polys, set_of, sets, gamma)))


# ---- NTT: k_ntt_pass ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("k", [1, 2, 10, 11, 12, 18, 20])
def test_ntt_chain(eng, k):
    """position 0 of the first pass's tile starts as r - 1 and adds H at every stage: 1.5 r + 0.5 r (m - 1), 6.5 r for the
    eleven stages of a single pass.  The input is zero off the stride of that pass, so the transform has period 2^m and is
    the transform of the 2^m chain values."""
    n = 1 << k
    for h in (FE.H_PLUS, FE.H_MINUS):
        x, m = FE.ntt_chain(k, h)
        small, _ = FE.ntt_chain_small(k, h)
        a = np.zeros((n, 4), dtype=np.uint64)
        for i, v in x.items():
            a[i] = _rows([v])[0]
        assert np.array_equal(eng.ntt_limbs(a), np.tile(_rows(NO.ntt(small)), (n >> m, 1))), ("forward", h == FE.H_PLUS)
        scale = pow(1 << (k - m), -1, R)  # intt divides by n, the chain's own inverse transform by 2^m
        want = [v * scale % R for v in NO.intt(small)]
        assert np.array_equal(eng.intt_limbs(a), np.tile(_rows(want), (n >> m, 1))), ("inverse", h == FE.H_PLUS)


@pytest.mark.parametrize("k", [11, 12])
def test_ntt_whole_vectors_of_extremes(eng, k):
    n = 1 << k
    vectors = {"H+": [FE.H_PLUS] * n, "H+ H-": [FE.H_PLUS, FE.H_MINUS] * (n // 2),
               "D+ D-": [FE.d_plus(0x73EC), FE.d_minus(0x73EC)] * (n // 2), "digit patterns": _digit_pattern(n)}
    for name, v in vectors.items():
        a = _rows(v)
        assert np.array_equal(eng.ntt_limbs(a), _rows(NO.ntt(v))), name
        assert np.array_equal(eng.intt_limbs(a), _rows(NO.intt(v))), name


# ---- barycentric evaluation: k_bary_partial, k_bary_finish ----------------------------------------------------------------


@pytest.mark.parametrize("k", [10, 17])
def test_barycentric_sums_of_half_values(eng, k):
    """f_i = H (z - w^i) / w^i makes every term of the sum H.  Four of them are -2, so that input fills the run sums only;
    H / 4 and H / 1024 per term fill the sums over the lanes of a tile and over the tiles."""
    n = 1 << k
    w = NO.domain_root(k)
    wi = pow(w, -1, R)
    pts, inv = [1] * n, [1] * n
    for i in range(1, n):
        pts[i], inv[i] = pts[i - 1] * w % R, inv[i - 1] * wi % R
    cases = [(FE.H_PLUS, 1, _random(31)), (FE.H_MINUS, 1, MULTS[3]), (FE.H_PLUS, 4, MULTS[0]), (FE.H_MINUS, 4, _random(32)),
             (FE.H_PLUS, 1024, MULTS[4]), (FE.H_MINUS, 1024, _random(33))]
    if k == 17:  # the run sums are a lane's own and were filled at k = 10; the oracle is O(n) big-integer steps per polynomial
        cases = [cases[2], cases[5]]
    evals, zs = [], []
    for h, scale, z in cases:
        target = h * pow(scale, -1, R) % R
        evals.append([target * (z - p) % R * q % R for p, q in zip(pts, inv)])
        zs.append(z)
    evals.append([FE.d_plus(0x73EC), FE.d_minus(0x73EC)] * (n // 2))
    zs.append(_random(34))
    got = eng.evaluate_evaluations_batch(np.stack([_rows(e) for e in evals]), [K.Scalar(z) for z in zs])
    for b, (e, z) in enumerate(zip(evals, zs)):
        assert got[b].v == _value(NO.barycentric_eval(e, z)), b


# ---- quotient scans: poly_kernels.hip, cell_kernels.hip, blobproof_kernels.hip ----------------------------------------------


def _scan_inputs(n):
    return {"D+": [FE.d_plus(0)] * n, "D-": [FE.d_minus(0x73EC)] * n, "alternating": [FE.d_plus(0x73EC), FE.d_minus(0)] * (n // 2 + 1),
            "patterns": _digit_pattern(n)}


@pytest.mark.parametrize("n", [4096, 4097, 16385])
def test_quotient_scan_of_digit_extremal_coefficients(eng, n):
    for name, f in _scan_inputs(n).items():
        f = f[:n]
        a = _rows(f)
        for z in MULTS:  # MULTS[0] is the z with z 2^270 = H+
            q, fz = CO.quotient(f, z)
            got = eng.quotient_limbs(a, K.Scalar(z), K.Scalar(_value(fz)))
            assert np.array_equal(got, _rows(q)), (name, hex(z))


@pytest.mark.parametrize("k", [2, 16])
def test_quotient_by_several_points_of_digit_extremal_coefficients(eng, k):
    n = 4097
    zs = (MULTS + [_random(40 + i) for i in range(10)])[:k]
    for name, f in _scan_inputs(n).items():
        f = f[:n]
        ys = [K.Scalar(_value(TO.poly_eval(f, z))) for z in zs]
        q, _ = PO.poly_div_vanishing(f, zs)
        got = eng.quotient_points_limbs(_rows(f), [K.Scalar(z) for z in zs], ys)
        assert np.array_equal(got, _rows(q)), name


def test_cell_quotients_of_digit_extremal_coefficients(eng):
    n, K_, t = 100, 8, 2
    for name, f in _scan_inputs(n).items():
        f = f[:n]
        got = eng.quotient_cells_limbs(_rows(f), K_, t)
        for j in range((1 << K_) >> t):
            assert np.array_equal(got[j], _rows(CL.stride_quotient(f, 1 << t, CL.cell_root(K_, t, j)))), (name, j)


def test_blob_openings_of_digit_extremal_coefficients(srs):
    n = 4096
    inputs = _scan_inputs(n)
    blobs, zs, coeffs = [], [], []
    for i, (name, f) in enumerate(inputs.items()):
        c = [_value(x) for x in f[:n]]  # the wire carries values; the device makes the images
        coeffs.append(c)
        blobs.append(W.fr_list_be(NO.ntt(c)))
        zs.append(MULTS[i])
    ys, proofs = srs.blobs_open_at_bytes(b"".join(blobs), n, b"".join(z.to_bytes(32, "big") for z in zs))
    want = [BP.open_at(O, b, K.KZG_ORDER_NATURAL, z, S, coeffs=c) for b, z, c in zip(blobs, zs, coeffs)]
    assert ys == b"".join(w[0] for w in want)
    assert proofs == b"".join(w[1] for w in want)


# ---- verifier sums: k_vc_fr_sum, k_vc_fr_twist -----------------------------------------------------------------------------


@pytest.mark.parametrize("weights", ["random", "extremal"])
def test_verifier_fold_of_33_records_on_one_cell(srs, weights):
    """33 records on one cell id: two full folds of 16 and one more, then a fold of three.  v_t = H / rho_t makes every
    product of the first level H; H / 16 makes every stored fold H"""
    K_, t = 5, 2
    l, G2 = 1 << t, [K.srs_g2_at(T.BENCH_SECRET_BE, i) for i in range((1 << t) + 1)]
    rnd = random.Random(50)
    c = np.stack([K.scalars_to_limbs([rnd.randrange(R) for _ in range(20)]) for _ in range(2)])
    _, proofs = srs.cells_and_proofs_fk20(c, K_, t, cells=False)
    coms = np.stack([srs.commit_limbs(c[b]).p1 for b in range(2)])
    k, cell = 33, 3
    idx = np.array([i % 2 for i in range(k)], dtype=np.uint32)
    ids = np.full(k, cell, dtype=np.uint32)
    prf = np.stack([proofs[int(b)][cell].p1 for b in idx])
    rho = [rnd.randrange(1, R) for _ in range(k)] if weights == "random" else (MULTS * 6)[:k]
    targets = [FE.H_PLUS, FE.H_MINUS, FE.H_PLUS * pow(16, -1, R) % R, FE.H_MINUS * pow(16, -1, R) % R]  # one per column
    images = [[targets[i] * pow(w, -1, R) % R for i in range(l)] for w in rho]
    vals = np.stack([_rows(row) for row in images])
    lhs, rhs, _ = srs.verify_cells_lincomb(coms, idx, ids, vals, prf, K_, t, G2, [K.Scalar(x) for x in rho])
    pt = lambda a: T.g1_from_blst_p1_limbs([int(x) for x in a])  # noqa: E731
    want_l, want_r = VO.g1_sides(K_, t, [pt(x) for x in coms], [int(x) for x in idx], [int(x) for x in ids],
                                 [[_value(x) for x in row] for row in images], [pt(p) for p in prf], rho,
                                 T.srs_g1(T.BENCH_SECRET_BE, l))
    assert lhs.compress() == T.g1_compress(want_l) and rhs.compress() == T.g1_compress(want_r)


# ---- recovery and the FK20 Fr stages: a canonical value after every product, so only the first level matters ----------------


def test_recovery_from_digit_extremal_cells(srs):
    K_, t, n = 6, 2, 32
    l, ids = 1 << t, [5, 0, 15, 2, 9, 7, 12, 3]  # exactly n / l cells: any values are the cells of one polynomial
    received = [_digit_pattern(l, 3 * j) for j in range(len(ids))]
    poly, ok = RO.decode(n, K_, t, ids, received)
    assert ok
    co, ce, _ = srs.recover_cells_and_proofs(n, K_, t, ids, np.stack([_rows(c) for c in received])[None], proofs=False)
    assert np.array_equal(co[0], _rows(poly))
    assert np.array_equal(ce[0], _rows(CL.cells(poly, K_, t)))


def test_fk20_of_digit_extremal_coefficients(srs):
    K_, t, n = 6, 2, 32
    f = _digit_pattern(n)
    cells, proofs = srs.cells_and_proofs_fk20(_rows(f)[None], K_, t)
    assert np.array_equal(cells[0], _rows(CL.cells(f, K_, t)))
    want_cells, want = srs.cells_and_proofs_limbs(_rows(f), K_, t)
    assert np.array_equal(cells[0], want_cells)
    assert np.array_equal(np.stack([p.p1 for p in proofs[0]]), np.stack([p.p1 for p in want]))
