"""GPU: the data-availability family (kzg_cells_and_proofs_fk20, kzg_g1_dft, kzg_recover_cells_and_proofs,
kzg_verify_cells_batch / kzg_verify_cells_lincomb) at degenerate setups, structured coefficients and adversarial points,
against the trapdoor oracle of tests/trapdoor_oracle.py: with the secret s known, every proof is [q_j(s)]G and every G1
DFT output of an SRS is [(s^m - 1) / (s w^j - 1)]G, so each output is checked on its own rather than against another
path of the library.

The branches reached: the doubling and the cancellation of the complete additions (xyzz30_add) in the G1 butterflies,
the comb tables, the fold tree and the segmented sums; infinity bases in the comb tables and their normalisation
(k_normalize); the edges of the host's GLV split (glv_split) and the top bit of the verifier's ladder (g1_mul_glv); the
subgroup check of k_vc_ladder on G1 points shifted by torsion."""
import ctypes as C
import random

import numpy as np
import pytest

import bigint_twin as T
import cells_oracle as CO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import trapdoor_oracle as TO
import verify_cells_oracle as VO

pytestmark = pytest.mark.gpu
R = K.R_MODULUS
S_BENCH = T.fr_from_be_bytes(T.BENCH_SECRET_BE)
SG = 0x1234567890ABCDEF  # a generic secret for the G1 DFT
LAMBDA = VO.LAMBDA
OMEGA3 = pow(7, (R - 1) // 3, R)

# (n, log N, log l): l in {1, 8, 64}, N up to 2^13; m = n / l = 64 and L = 128 in each, so w_L is one secret for all
SHAPES = [(4096, 13, 6), (512, 10, 3), (64, 7, 0)]
SECRETS = ["0", "1", "r-1", "omega3", "2", "w_N^5", "w_l", "w_L"]


def _secret(name, K_, t):
    return {"0": 0, "1": 1, "r-1": R - 1, "omega3": OMEGA3, "2": 2, "w_N^5": pow(NO.domain_root(K_), 5, R),
            "w_l": NO.domain_root(t), "w_L": NO.domain_root(7)}[name]


def _structured(n, l):
    """(label, coefficients): random, zero, constant 1, all r - 1, one-hot at c_0, c_(l-1), c_l, c_(n-1), alternating +-1"""
    rnd = random.Random(n + l)
    out = [("random", [rnd.randrange(R) for _ in range(n)]), ("zero", [0] * n), ("ones", [1] * n), ("r-1", [R - 1] * n)]
    for i in (0, l - 1, l, n - 1):
        c = [0] * n
        c[i] = 1
        out.append(("onehot %d" % i, c))
    out.append(("alternating", [1 if i % 2 == 0 else R - 1 for i in range(n)]))
    return out


def _stack(points):
    return np.stack([p.p1 for p in points]) if points else np.zeros((0, 18), np.uint64)


def _limbs(pt, z=1):
    return np.array(T.g1_to_blst_p1_limbs(pt, z), dtype=np.uint64)


class _Points:
    """[v]G as compressed bytes, one oracle multiplication per distinct v"""

    def __init__(self, oracle):
        self.oracle, self.memo = oracle, {}

    def __call__(self, v):
        v %= R
        if v not in self.memo:
            self.memo[v] = TO.g1_scalar(self.oracle, v)
        return self.memo[v]


@pytest.fixture(scope="module")
def gpts(oracle):
    return _Points(oracle)


@pytest.fixture(scope="module")
def setups():
    """one engine per secret (4096 SRS points: n' - l for every shape, and l for the verifier)"""
    made = {}

    def get(s):
        if s not in made:
            made[s] = K.SetupArtifactsGenerator(TO.secret_be(s)).take(4096)
        return made[s]

    yield get
    for e in made.values():
        e.close()


_EXPECT = {}


def _expected(vals, K_, t, s):
    key = (tuple(vals), K_, t, s)
    if key not in _EXPECT:
        _EXPECT[key] = TO.cell_proof_scalars_fast(vals, K_, t, s)
    return _EXPECT[key]


_CELLS = {}


def _cells(vals, K_, t):
    key = (tuple(vals), K_, t)
    if key not in _CELLS:
        _CELLS[key] = CO.cells(vals, K_, t)
    return _CELLS[key]


def _assert_proofs(gpts, proofs, vals, K_, t, s, what):
    q = _expected(vals, K_, t, s)
    for j, p in enumerate(proofs):
        assert p.compress() == gpts(q[j]), (what, j)


# ---- degenerate setups: FK20, the verifier ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SECRETS)
def test_fk20_and_verify_at_degenerate_secret(setups, gpts, monkeypatch, name):
    """Every FK20 proof of the structured batch equals [q_j(s)]G, with the comb tables kept and again streamed
    (KZG_FK20_TABLE_MB=0).  s = 1 with constant coefficients adds equal points at every fold level (doubling); s = r - 1
    with alternating coefficients makes them cancel; s = 0 and s = w_L give infinity bases to the comb tables and their
    normalisation; s = w_N^5 and s = w_l put s on a cell (s^l = a_j, a zero vanishing value).  The honest records pass
    kzg_verify_cells_batch ([s^l]G2 is infinity for s = 0), and kzg_verify_cells_lincomb's sides are the scalar sides."""
    kept = {}
    for n, K_, t in SHAPES:
        s = _secret(name, K_, t)
        e = setups(s)
        polys = _structured(n, 1 << t)
        c = np.stack([K.scalars_to_limbs(v) for _, v in polys])
        cells, proofs = e.cells_and_proofs_fk20(c, K_, t)
        kept[(n, K_, t)] = (s, c, proofs)
        for b, (label, vals) in enumerate(polys):
            assert K.limbs_to_scalars(cells[b]) == _cells(vals, K_, t), (label, K_, t)
            _assert_proofs(gpts, proofs[b], vals, K_, t, s, (name, label, K_, t))
        _verify_honest(e, gpts, polys, c, cells, proofs, K_, t, s)
    monkeypatch.setenv("KZG_FK20_TABLE_MB", "0")
    for (n, K_, t), (s, c, proofs) in kept.items():
        e = K.SetupArtifactsGenerator(TO.secret_be(s)).take(4096)
        try:
            _, streamed = e.cells_and_proofs_fk20(c, K_, t, cells=False)
        finally:
            e.close()
        for b in range(len(proofs)):
            assert np.array_equal(_stack(streamed[b]), _stack(proofs[b])), (name, K_, t, b)


def _verify_honest(e, gpts, polys, c, cells, proofs, K_, t, s):
    l, M = 1 << t, (1 << K_) >> t
    g2 = [K.srs_g2_at(TO.secret_be(s), i) for i in range(l + 1)]
    coms = [e.commit_limbs(c[b]) for b in range(len(polys))]
    for (label, vals), cm in zip(polys, coms):
        assert cm.compress() == gpts(TO.poly_eval(vals, s)), label
    batch = len(polys)
    idx = np.repeat(np.arange(batch, dtype=np.uint32), M)
    ids = np.tile(np.arange(M, dtype=np.uint32), batch)
    vals = np.ascontiguousarray(cells.reshape(batch * M, l, 4))
    prf = np.stack([p.p1 for b in range(batch) for p in proofs[b]])
    assert e.verify_cells_batch(coms, idx, ids, vals, prf, K_, t, g2)
    # a few records through the lincomb hook: the cell s lies on (if any), cell 0, the last cell, random weights
    rows = sorted({0, 5 % M, M - 1, M + 5 % M, 3 * M + 1 % M, (batch - 1) * M + M // 2})
    rnd = random.Random(K_ * 100 + t)
    w = [rnd.randrange(R) for _ in rows]
    ri, rj, rv, rp = idx[rows], ids[rows], vals[rows], prf[rows]
    lhs, rhs, ok = e.verify_cells_lincomb(coms, ri, rj, rv, rp, K_, t, g2, [K.Scalar(x) for x in w])
    assert ok
    q = [_expected(polys[int(b)][1], K_, t, s)[int(j)] for b, j in zip(ri, rj)]
    want_l, want_r = VO.scalar_sides(K_, t, [TO.poly_eval(v, s) for _, v in polys], [int(x) for x in ri], [int(x) for x in rj],
                                     [K.limbs_to_scalars(v) for v in rv], q, w, s)
    assert lhs.compress() == gpts(want_l) and rhs.compress() == gpts(want_r)


# ---- recovery erasure patterns ------------------------------------------------------------------------------------------------
def _patterns(M, n, l):
    need = -(-n // l)
    rnd = random.Random(M)
    exact = [0, M - 1] + rnd.sample(range(1, M - 1), need - 2)
    return {"odd missing": list(range(0, M, 2)), "first half missing": list(range(M // 2, M)),
            "cell 0 missing": list(range(1, M)), "exactly n/l": exact}


@pytest.mark.parametrize("name", ["0", "r-1", "w_N^5", "w_L"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]])
def test_recovery_erasure_patterns(setups, gpts, name, shape):
    """kzg_recover_cells_and_proofs of the zero polynomial, all r - 1 and a one-hot top coefficient from every odd cell
    missing, the first half missing, only cell 0 missing and exactly n/l cells (0 and M - 1 among them): coefficients
    against the originals, cells against cells_oracle, proofs against [q_j(s)]G -- the recovered proofs run FK20 on
    recovered coefficients whose folds double (all r - 1) or are mostly infinity (zero, one-hot)"""
    n, K_, t = shape
    l, M = 1 << t, (1 << K_) >> t
    s = _secret(name, K_, t)
    e = setups(s)
    top = [0] * n
    top[n - 1] = 1
    polys = [[0] * n, [R - 1] * n, top]
    c = np.stack([K.scalars_to_limbs(p) for p in polys])
    full = np.stack([K.scalars_to_limbs(_cells(p, K_, t)) for p in polys])
    for label, ids in _patterns(M, n, l).items():
        rx = np.ascontiguousarray(full.reshape(3, M, l, 4)[:, ids])
        co, ce, pr = e.recover_cells_and_proofs(n, K_, t, ids, rx)
        assert np.array_equal(co, c), label
        assert np.array_equal(ce, full), label
        for b, p in enumerate(polys):
            _assert_proofs(gpts, pr[b], p, K_, t, s, (name, label, b))


# ---- the G1 DFT ----------------------------------------------------------------------------------------------------------------
def _dft_raw(e, arr, inverse=False):
    """kzg_g1_dft straight on an (m, 18) array, no per-row Python objects"""
    a = np.ascontiguousarray(arr, dtype=np.uint64)
    out = np.zeros_like(a)
    rc = K.load_library().kzg_g1_dft(e._h, a.ctypes.data_as(C.c_void_p), a.shape[0], 1 if inverse else 0,
                                     out.ctypes.data_as(C.c_void_p))
    assert rc == K.KZG_OK, K.load_library().kzg_last_error(e._h)
    return out


def _compress_row(row):
    return K.G1Point(row).compress()


@pytest.fixture(scope="module")
def dft_eng():
    e = K.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("k", range(14))
def test_g1_dft_structured_inputs(dft_eng, gpts, k):
    """m = 2^k, every output: all infinity; one-hot (m - 1 for k <= 10, m / 4 above); a constant P (every butterfly
    adds equal points); +-P alternating (they cancel); a pure frequency (the SRS of s = w^-f: m G at f, infinity
    elsewhere, so each stage meets both); the SRS of a generic secret given with Jacobian Z != 1, against the closed
    form, and its inverse round trip"""
    m = 1 << k
    e = dft_eng
    w = NO.domain_root(k)
    e.srs_generate(TO.secret_be(SG), m)
    srs = e.srs_read(0, m)
    P = srs[min(1, m - 1)]  # [SG]G (G when m = 1)
    a = SG if m > 1 else 1

    def check(out, scalars, what):
        for j in range(m):
            v = scalars(j) % R
            if v == 0:
                assert not out[j].any(), (what, k, j)
            else:
                assert _compress_row(out[j]) == gpts(v), (what, k, j)

    zero = np.zeros((m, 18), np.uint64)
    assert not _dft_raw(e, zero).any() and not _dft_raw(e, zero, inverse=True).any()
    i0 = m - 1 if k <= 10 else m // 4
    hot = zero.copy()
    hot[i0] = P
    check(_dft_raw(e, hot), lambda j: a * pow(w, i0 * j, R), "one-hot")
    check(_dft_raw(e, np.tile(P, (m, 1))), lambda j: m * a if j == 0 else 0, "constant")
    if m > 1:
        neg = _limbs(T.g1_neg(T.g1_from_blst_p1_limbs([int(x) for x in P])))
        alt = np.stack([P if i % 2 == 0 else neg for i in range(m)])
        check(_dft_raw(e, alt), lambda j: m * a if j == m // 2 else 0, "alternating")
    f = m // 3
    e.srs_generate(TO.secret_be(pow(w, (m - f) % m, R)), m)
    check(_dft_raw(e, e.srs_read(0, m)), lambda j: m if j == f else 0, "pure frequency")
    # the SRS of SG with Z = 2 + i (Jacobian, not normalised)
    jac = np.stack([_limbs(T.g1_from_blst_p1_limbs([int(x) for x in row]), 2 + i) for i, row in enumerate(srs)])
    closed = TO.srs_dft_scalars(SG, m)
    out = _dft_raw(e, jac)
    check(out, lambda j: closed[j], "srs, Z != 1")
    assert np.array_equal(_dft_raw(e, out, inverse=True), srs)


@pytest.mark.parametrize("lg", [16, 20, 22])
def test_g1_dft_large_root_of_unity_setup(gpts, lg):
    """m = 2^16, 2^20 and 2^22 (the stated maximum) on srs_read arrays: the SRS of s = w_m^-j0 transforms to m G at j0
    and infinity at every other bin (every butterfly of the last stages cancels); a generic secret at sampled bins
    against the closed form, and the inverse round trip back to the SRS"""
    m = 1 << lg
    w = NO.domain_root(lg)
    j0 = 12345
    e = K.SetupArtifactsGenerator(TO.secret_be(pow(w, m - j0, R))).take(m)
    try:
        out = _dft_raw(e, e.srs_read(0, m))
        assert _compress_row(out[j0]) == gpts(m)
        out[j0] = 0
        assert not out.any()
        del out
        e.srs_generate(TO.secret_be(SG), m)
        srs = e.srs_read(0, m)
        out = _dft_raw(e, srs)
        num = (pow(SG, m, R) - 1) % R
        for j in sorted({0, 1, 2, m // 2, m - 1} | set(random.Random(lg).sample(range(m), 4))):
            v = num * pow((SG * pow(w, j, R) - 1) % R, R - 2, R) % R
            assert _compress_row(out[j]) == gpts(v), j
        assert np.array_equal(_dft_raw(e, out, inverse=True), srs)
    finally:
        e.close()


# ---- verifier weights and adversarial points (bench setup) ------------------------------------------------------------------
G2_BENCH = [K.srs_g2_at(T.BENCH_SECRET_BE, i) for i in range(5)]
VK, VT = 5, 2  # N = 32, l = 4, M = 8


@pytest.fixture(scope="module")
def vbatch(engines):
    """two polynomials of 20 coefficients: commitments, all cells and proofs on the bench setup"""
    e = engines.bench_srs(256)
    rnd = random.Random(77)
    polys = [[rnd.randrange(R) for _ in range(20)] for _ in range(2)]
    c = np.stack([K.scalars_to_limbs(p) for p in polys])
    cells, proofs = e.cells_and_proofs_fk20(c, VK, VT)
    coms = np.stack([e.commit_limbs(c[b]).p1 for b in range(2)])
    return e, polys, coms, cells.reshape(2, 8, 4, 4), proofs


def _pt(row):
    return T.g1_from_blst_p1_limbs([int(x) for x in row])


def _lincomb_vs_twin(vb, recs, weights):
    """recs: (b, j) records; compares both sides of kzg_verify_cells_lincomb with the twin's group law"""
    e, polys, coms, cells, proofs = vb
    ri = np.array([b for b, _ in recs], np.uint32)
    rj = np.array([j for _, j in recs], np.uint32)
    rv = np.stack([cells[b, j] for b, j in recs])
    rp = np.stack([proofs[b][j].p1 for b, j in recs])
    lhs, rhs, ok = e.verify_cells_lincomb(coms, ri, rj, rv, rp, VK, VT, G2_BENCH, [K.Scalar(x % R) for x in weights])
    assert ok
    want_l, want_r = VO.g1_sides(VK, VT, [_pt(cm) for cm in coms], [int(x) for x in ri], [int(x) for x in rj],
                                 [K.limbs_to_scalars(v) for v in rv], [_pt(p) for p in rp], weights,
                                 T.srs_g1(T.BENCH_SECRET_BE, 4))
    assert lhs.compress() == T.g1_compress(want_l) and rhs.compress() == T.g1_compress(want_r)
    return want_l, want_r


EDGE_WEIGHTS = [0, 1, R - 1, LAMBDA, LAMBDA - 1, LAMBDA + 1, 1 << 64, 1 << 127, 1 << 128]


def test_lincomb_edge_weights(vbatch):
    """weights at the edges of glv_split: r - 1 = lambda (lambda + 1) splits as k1 = 0, k2 = z^2 (bit 127 set, the
    ladder's top bit); lambda, lambda +- 1 (k2 = 1, k1 = 0 / lambda - 1 / 0 with a carry); 2^127, 2^128 (a remainder
    past 2^127 in the division, the `over` test); 0 and 1.  Each weight alone on one record, then all together"""
    for w in EDGE_WEIGHTS:
        _lincomb_vs_twin(vbatch, [(0, 3), (1, 5)], [w, 1])
        _lincomb_vs_twin(vbatch, [(0, 3)], [w])
    recs = [(b, j) for b in range(2) for j in range(8)][:len(EDGE_WEIGHTS)]
    _lincomb_vs_twin(vbatch, recs, EDGE_WEIGHTS)


def test_lincomb_cancelling_weights(vbatch):
    """a record given twice with weights w and r - w (its T_j and U_b cancel to infinity); every record of one cell
    weighted so that T_j = sum rho_t pi_t is infinity entering k_vc_cell_scale (the weights from the known secret)"""
    rnd = random.Random(5)
    for w in (1, R - 1, LAMBDA, 1 << 128, rnd.randrange(R)):
        _lincomb_vs_twin(vbatch, [(1, 6), (1, 6), (0, 2)], [w, R - w, 3])
        _lincomb_vs_twin(vbatch, [(1, 6), (1, 6)], [w, R - w])
    _, polys, _, _, _ = vbatch
    q0 = TO.cell_proof_scalars_fast(polys[0], VK, VT, S_BENCH, cells=[4])[4]
    q1 = TO.cell_proof_scalars_fast(polys[1], VK, VT, S_BENCH, cells=[4])[4]
    assert q0 and q1
    for w0 in (1, R - 1, rnd.randrange(R)):
        w1 = -w0 * q0 * pow(q1, R - 2, R) % R
        _lincomb_vs_twin(vbatch, [(0, 4), (1, 4), (0, 7)], [w0, w1, 2])
        _lincomb_vs_twin(vbatch, [(0, 4), (1, 4)], [w0, w1])


def test_torsion_shifted_points_are_rejected(vbatch):
    """a proof, a commitment or both equal to G1 + T for a point T of each prime order of the cofactor, and the order-3
    points (0, +-2) alone: kzg_verify_cells_batch refuses them as not in G1 (the subgroup check of k_vc_ladder)"""
    e, polys, coms, cells, proofs = vbatch
    lib = K.load_library()
    recs = [(b, j) for b in range(2) for j in range(8)]
    ri = np.array([b for b, _ in recs], np.uint32)
    rj = np.array([j for _, j in recs], np.uint32)
    rv = np.stack([cells[b, j] for b, j in recs])
    rp = np.stack([proofs[b][j].p1 for b, j in recs])
    assert e.verify_cells_batch(coms, ri, rj, rv, rp, VK, VT, G2_BENCH)

    def refused(cm, pr):
        with pytest.raises(K.KzgError) as ei:
            e.verify_cells_batch(cm, ri, rj, rv, pr, VK, VT, G2_BENCH)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        return lib.kzg_last_error(e._h)

    tors = TO.torsion_points()
    for q, tp in sorted(tors.items()):
        p2 = rp.copy()
        p2[11] = _limbs(T.g1_add(_pt(rp[11]), tp), 3)
        msg = refused(coms, p2)
        assert b"record 11" in msg and b"not in G1" in msg, q
        c2 = coms.copy()
        c2[1] = _limbs(T.g1_add(_pt(coms[1]), tp))
        msg = refused(c2, rp)
        assert b"commitment 1" in msg and b"not in G1" in msg, q
        assert b"not in G1" in refused(c2, p2), q
    for tp in TO.ORDER3:
        p2 = rp.copy()
        p2[0] = _limbs(tp, 2)
        msg = refused(coms, p2)
        assert b"record 0" in msg and b"not in G1" in msg
        c2 = coms.copy()
        c2[0] = _limbs(tp)
        msg = refused(c2, rp)
        assert b"commitment 0" in msg and b"not in G1" in msg
