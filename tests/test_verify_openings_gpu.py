"""GPU: kzg_evaluate_evaluations_batch, kzg_verify_openings_batch / _lincomb and kzg_verify_evaluations_batch (DESIGN.md
section 4.11): the barycentric values against kzg_ntt(inverse) + kzg_evaluate and the big-integer oracle, acceptance across
record layouts, rejection of each corruption, agreement with kzg_verify_proof, the two sides against the oracle, errors,
multi-device contexts, the evaluation-form verifier and concurrency."""
import random
import threading

import numpy as np
import pytest

import bigint_twin as T
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import trapdoor_oracle as TO
import verify_cells_oracle as VCO
import verify_openings_oracle as VO

pytestmark = pytest.mark.gpu
R = K.R_MODULUS
G2 = [K.srs_g2_at(T.BENCH_SECRET_BE, i) for i in range(2)]
S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)


@pytest.fixture(scope="module")
def eng():
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(4096)
    yield e
    e.close()


def _limbs(v):
    return K.scalars_to_limbs([v % R])[0]


def _scalar(row):
    return K.limbs_to_scalars(np.asarray(row, dtype=np.uint64).reshape(1, 4))[0]


def _random_images(rng, shape):
    """blst_fr images of uniformly random-looking field elements: any 256-bit value below r is one"""
    a = rng.integers(0, 1 << 63, size=shape + (4,), dtype=np.uint64)
    a[..., :3] |= rng.integers(0, 2, size=shape + (3,), dtype=np.uint64) << np.uint64(63)
    a[..., 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)  # below 2^254 < r
    return a


# ---- 1. evaluation -------------------------------------------------------------------------------------------------------
EVAL_SHAPES = [(n, b) for n in (1, 2, 4, 64, 4096) for b in (1, 3, 64)] + [(n, b) for n in (1 << 16, 1 << 20) for b in (1, 3)]


@pytest.mark.parametrize("n,batch", EVAL_SHAPES)
def test_evaluation_matches_interpolation_and_oracle(eng, n, batch):
    rng = np.random.default_rng(n * 131 + batch)
    rnd = random.Random(n * 7 + batch)
    k = NO.log2_exact(n)
    w = NO.domain_root(k)
    evals = _random_images(rng, (batch, n))
    coeffs = [eng.intt_limbs(evals[b]) for b in range(batch)]
    ints = {b: K.limbs_to_scalars(evals[b]) for b in range(batch) if n <= 4096 or b == 0}

    def check(ev, cf, zs, oracle_for):
        got = eng.evaluate_evaluations_batch(ev, [K.Scalar(z) for z in zs])
        for b in range(batch):
            want = eng.evaluate_limbs(cf[b], K.Scalar(zs[b]))
            assert got[b].v == want.v, (n, batch, b, zs[b])
        for b, vals in oracle_for.items():
            assert got[b].v == NO.barycentric_eval(vals, zs[b]), (n, batch, b)
            if n <= 64:
                assert got[b].v == VO.barycentric(vals, zs[b])

    kinds = [lambda b: rnd.randrange(R), lambda b: 0, lambda b: 1, lambda b: w, lambda b: pow(w, n // 2, R),
             lambda b: pow(w, n - 1, R), lambda b: (pow(w, rnd.randrange(n), R) + 1) % R]
    for kind in kinds:
        check(evals, coeffs, [kind(b) for b in range(batch)], ints if n <= 4096 else {})
    # in-domain and out-of-domain points mixed in one call (against the oracle at every size, polynomial 0 at the large ones)
    check(evals, coeffs, [kinds[(b + 3) % len(kinds)](b) for b in range(batch)], ints)
    # values all zero, values all r - 1
    zero = np.zeros_like(evals)
    top = np.broadcast_to(_limbs(R - 1), evals.shape).copy()
    zs = [rnd.randrange(R) if b % 2 == 0 else pow(w, b % n, R) for b in range(batch)]
    got = eng.evaluate_evaluations_batch(zero, [K.Scalar(z) for z in zs])
    assert all(v.v == 0 for v in got)
    got = eng.evaluate_evaluations_batch(top, [K.Scalar(z) for z in zs])
    assert all(v.v == R - 1 for v in got)  # the constant r - 1


# ---- records from the library's own provers ------------------------------------------------------------------------------
class Records:
    """openings of `polys` random polynomials of n coefficients: record t = (polynomial idx[t], point zs[t])"""

    def __init__(self, e, n, polys, idx, zs, seed, evaluation_form=False):
        rnd = random.Random(seed)
        self.coeffs = [[rnd.randrange(R) for _ in range(n)] for _ in range(polys)]
        self.limbs = [K.scalars_to_limbs(c) for c in self.coeffs]
        self.coms = np.stack([e.commit_limbs(l).p1 for l in self.limbs])
        self.idx = np.array(idx, dtype=np.uint32)
        self.zs = [z % R for z in zs]
        self.ys = [TO.poly_eval(self.coeffs[b], z) for b, z in zip(idx, self.zs)]
        prf = []
        for b, z, y in zip(idx, self.zs, self.ys):
            if n == 1:
                prf.append(np.zeros(18, dtype=np.uint64))  # a constant has the quotient zero
            elif evaluation_form:
                prf.append(e.open_evaluations_limbs(e.ntt_limbs(self.limbs[b]), K.Scalar(z), K.Scalar(y)).p1)
            else:
                prf.append(e.open_limbs(self.limbs[b], K.Scalar(z), K.Scalar(y)).p1)
        self.prf = np.stack(prf)

    def verify(self, e, rows=None, coms=None, idx=None, zs=None, ys=None, prf=None):
        rows = list(range(len(self.idx))) if rows is None else list(rows)
        pick = lambda a: [a[i] for i in rows]  # noqa: E731
        return e.verify_openings_batch(self.coms if coms is None else coms, pick(self.idx) if idx is None else idx,
                                       [K.Scalar(z) for z in (pick(self.zs) if zs is None else zs)],
                                       [K.Scalar(y) for y in (pick(self.ys) if ys is None else ys)],
                                       np.stack(pick(self.prf)) if prf is None else prf, G2)

    def singles(self, ys=None, zs=None, idx=None, prf=None, coms=None):
        ys, zs = self.ys if ys is None else ys, self.zs if zs is None else zs
        idx, prf, coms = self.idx if idx is None else idx, self.prf if prf is None else prf, self.coms if coms is None else coms
        return [K.verify_proof(K.G1Point(coms[b]), K.G1Point(p), K.Scalar(z), K.Scalar(y), G2[1])
                for b, z, y, p in zip(idx, zs, ys, prf)]


# ---- 2. acceptance -------------------------------------------------------------------------------------------------------
def test_openings_from_both_provers_shuffled_and_duplicated(eng):
    rnd = random.Random(1)
    idx = [rnd.randrange(4) for _ in range(24)]
    zs = [rnd.randrange(R) for _ in range(24)]
    for form in (False, True):
        r = Records(eng, 64, 4, idx, zs, 10 + form, evaluation_form=form)
        assert r.verify(eng)
        rows = list(range(24)) + [3, 3, 7]
        rnd.shuffle(rows)
        assert r.verify(eng, rows=rows)
        assert r.verify(eng, rows=[5])  # k = 1
    assert eng.verify_openings_batch([], [], [], [], [], G2)  # k = 0
    lhs, rhs, ok = eng.verify_openings_lincomb([], [], [], [], [], G2, [])
    assert ok and not lhs.p1.any() and not rhs.p1.any()


def test_many_commitments_at_one_point_and_one_commitment_at_many(eng):
    rnd = random.Random(2)
    z = rnd.randrange(R)
    shared = Records(eng, 16, 256, list(range(256)), [z] * 256, 20)
    assert shared.verify(eng)
    ys = list(shared.ys)
    ys[200] = (ys[200] + 1) % R
    assert not shared.verify(eng, ys=ys)
    one = Records(eng, 300, 1, [0] * 256, [rnd.randrange(R) for _ in range(256)], 21)  # every record its own point
    assert one.verify(eng)
    zs = list(one.zs)
    zs[17] = (zs[17] + 1) % R
    assert not one.verify(eng, zs=zs)


def test_constant_and_zero_polynomials(eng):
    rnd = random.Random(3)
    const = Records(eng, 1, 3, [0, 1, 2, 1], [rnd.randrange(R) for _ in range(4)], 30)
    assert not const.prf.any()  # infinity proofs
    assert const.verify(eng)
    ys = list(const.ys)
    ys[2] = (ys[2] + 1) % R
    assert not const.verify(eng, ys=ys)
    zero_com = np.zeros((1, 18), dtype=np.uint64)  # the zero polynomial: infinity commitment, value zero, infinity proof
    zero_prf = np.zeros((2, 18), dtype=np.uint64)
    zs = [K.Scalar(rnd.randrange(R)) for _ in range(2)]
    assert eng.verify_openings_batch(zero_com, [0, 0], zs, [K.Scalar(0)] * 2, zero_prf, G2)
    assert not eng.verify_openings_batch(zero_com, [0, 0], zs, [K.Scalar(0), K.Scalar(1)], zero_prf, G2)


# ---- 3. rejection --------------------------------------------------------------------------------------------------------
def test_each_corruption_is_rejected(eng):
    rnd = random.Random(4)
    idx = [t % 3 for t in range(12)]
    r = Records(eng, 50, 3, idx, [rnd.randrange(R) for _ in range(12)], 40)
    assert r.verify(eng)
    ys = list(r.ys)
    ys[5] = (ys[5] + 1) % R
    assert not r.verify(eng, ys=ys)
    zs = list(r.zs)
    zs[6] = (zs[6] + 1) % R
    assert not r.verify(eng, zs=zs)
    p2 = r.prf.copy()
    p2[[2, 9]] = p2[[9, 2]]
    assert not r.verify(eng, prf=p2)
    i2 = list(idx)
    i2[4] = (i2[4] + 1) % 3
    assert not r.verify(eng, idx=i2)
    p3 = r.prf.copy()
    neg = T.g1_neg(T.g1_from_blst_p1_limbs([int(x) for x in p3[7]]))
    p3[7] = np.array(T.g1_to_blst_p1_limbs(neg), dtype=np.uint64)
    assert not r.verify(eng, prf=p3)


def test_cancelling_pair_is_sharp(eng):
    rnd = random.Random(5)
    z = rnd.randrange(R)
    r = Records(eng, 20, 1, [0, 0], [z, z], 50)
    bad = [(r.ys[0] + 9) % R, (r.ys[1] - 9) % R]
    args = (r.coms, r.idx, [K.Scalar(z)] * 2, [K.Scalar(y) for y in bad], r.prf, G2)
    lhs, rhs, ok = eng.verify_openings_lincomb(*args, [K.Scalar(5), K.Scalar(5)])
    assert ok  # equal weights cancel the two errors: the case is sharp
    lhs, rhs, ok = eng.verify_openings_lincomb(*args, [K.Scalar(5), K.Scalar(6)])
    assert not ok
    assert not eng.verify_openings_batch(*args)


# ---- 4. agreement with kzg_verify_proof ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_agrees_with_verify_proof(eng, seed):
    rnd = random.Random(100 + seed)
    idx = [rnd.randrange(8) for _ in range(64)]
    r = Records(eng, 32, 8, idx, [rnd.randrange(R) for _ in range(64)], 60 + seed)
    bad = set() if seed == 0 else set(rnd.sample(range(64), rnd.randrange(1, 6)))
    ys = [(y + 1) % R if t in bad else y for t, y in enumerate(r.ys)]
    singles = r.singles(ys=ys)
    assert singles == [t not in bad for t in range(64)]
    assert r.verify(eng, ys=ys) == all(singles)


# ---- 5. the two sides ----------------------------------------------------------------------------------------------------
def test_lincomb_matches_oracle(eng):
    rnd = random.Random(6)
    z = rnd.randrange(R)
    idx = [0, 1, 1, 0, 1, 0, 1]
    zs = [z, z, rnd.randrange(R), rnd.randrange(R), z, 0, 1]
    r = Records(eng, 12, 2, idx, zs, 70)
    pt = lambda a: T.g1_from_blst_p1_limbs([int(x) for x in a])  # noqa: E731
    families = [[0, 1, R - 1, rnd.getrandbits(255) % R, VCO.glv_weight(rnd.getrandbits(64), rnd.getrandbits(64)), 1, 0],
                [VCO.glv_weight(rnd.getrandbits(64), rnd.getrandbits(64)) for _ in idx],
                [rnd.getrandbits(255) % R for _ in idx]]
    for weights in families:
        lhs, rhs, ok = eng.verify_openings_lincomb(r.coms, r.idx, [K.Scalar(v) for v in zs], [K.Scalar(y) for y in r.ys], r.prf,
                                                   G2, [K.Scalar(x) for x in weights])
        assert ok
        want_l, want_r = VO.g1_sides([pt(c) for c in r.coms], idx, zs, r.ys, [pt(p) for p in r.prf], weights)
        assert np.array_equal(lhs.p1, np.array(T.g1_to_blst_p1_limbs(want_l), dtype=np.uint64))
        assert np.array_equal(rhs.p1, np.array(T.g1_to_blst_p1_limbs(want_r), dtype=np.uint64))
        # and through the trapdoor: both sides are [v]G
        coms, prfs, ys = VO.trapdoor_records(r.coeffs, idx, zs, S)
        sl, sr = VO.scalar_sides(coms, idx, zs, ys, prfs, weights)
        assert lhs.compress() == T.g1_compress(T.g1_mul(T.G1, sl)) and rhs.compress() == T.g1_compress(T.g1_mul(T.G1, sr))


# ---- 6. errors -----------------------------------------------------------------------------------------------------------
def _status(fn):
    with pytest.raises(K.KzgError) as ei:
        fn()
    return ei.value.status


def test_errors(eng):
    rnd = random.Random(7)
    idx = [t % 2 for t in range(10)]
    r = Records(eng, 30, 2, idx, [rnd.randrange(R) for _ in range(10)], 80)
    lib = K.load_library()
    last = lambda: lib.kzg_last_error(eng._h)  # noqa: E731
    zl = np.stack([_limbs(z) for z in r.zs])
    yl = np.stack([_limbs(y) for y in r.ys])
    call = lambda coms=r.coms, idx=r.idx, zs=zl, ys=yl, prf=r.prf, g2=G2: eng.verify_openings_batch(  # noqa: E731
        coms, idx, zs, ys, prf, g2)
    assert call()
    INV = K.KZG_ERR_INVALID_ARG
    off = r.prf.copy()
    off[6, 6] ^= np.uint64(1)
    assert _status(lambda: call(prf=off)) == INV and b"record 6" in last() and b"curve" in last()
    coff = r.coms.copy()
    coff[1, 6] ^= np.uint64(1)
    assert _status(lambda: call(coms=coff)) == INV and b"commitment 1" in last() and b"curve" in last()
    for q, tp in TO.torsion_points().items():  # on the curve, outside G1: the proof shifted by a torsion point
        ng = r.prf.copy()
        shifted = T.g1_add(T.g1_from_blst_p1_limbs([int(x) for x in ng[3]]), tp)
        ng[3] = np.array(T.g1_to_blst_p1_limbs(shifted, 5), dtype=np.uint64)
        assert _status(lambda: call(prf=ng)) == INV and b"record 3" in last() and b"not in G1" in last(), q
        cg = r.coms.copy()
        cg[0] = np.array(T.g1_to_blst_p1_limbs(T.g1_add(T.g1_from_blst_p1_limbs([int(x) for x in cg[0]]), tp)), dtype=np.uint64)
        assert _status(lambda: call(coms=cg)) == INV and b"commitment 0" in last() and b"not in G1" in last(), q
    big_p = r.prf.copy()
    big_p[2, :6] = np.array([0xFFFFFFFFFFFFFFFF] * 6, dtype=np.uint64)  # x >= p
    assert _status(lambda: call(prf=big_p)) == INV and b"record 2" in last()
    big = np.array([0xFFFFFFFFFFFFFFFF] * 4, dtype=np.uint64)
    by = yl.copy()
    by[4] = big
    assert _status(lambda: call(ys=by)) == INV and b"record 4" in last()
    bz = zl.copy()
    bz[8] = big
    assert _status(lambda: call(zs=bz)) == INV and b"record 8" in last()
    bi = r.idx.copy()
    bi[0] = 2
    assert _status(lambda: call(idx=bi)) == INV and b"record 0" in last()
    g2_bad = [g.copy() for g in G2]
    g2_bad[1][3] ^= np.uint64(1)
    assert _status(lambda: call(g2=g2_bad)) == INV
    ok = K.C.c_int(0)
    null = lambda **kw: lib.kzg_verify_openings_batch(  # noqa: E731
        eng._h, kw.get("c", K._ptr(r.coms)), 2, kw.get("i", K._ptr(r.idx)), kw.get("z", K._ptr(zl)), kw.get("y", K._ptr(yl)),
        kw.get("p", K._ptr(r.prf)), 10, kw.get("g", K._ptr(np.stack(G2))), 288, kw.get("v", K.C.byref(ok)))
    assert null() == K.KZG_OK and ok.value == 1
    for name in "cizypgv":
        assert null(**{name: None}) == INV, name
    # evaluation: sizes, pointers, values
    ev = _random_images(np.random.default_rng(1), (2, 8))
    z2 = np.stack([_limbs(5), _limbs(6)])
    out = np.zeros((2, 4), dtype=np.uint64)
    ee = lambda e=ev, n=8, b=2, st=8, z=z2, o=out: lib.kzg_evaluate_evaluations_batch(  # noqa: E731
        eng._h, None if e is None else K._ptr(e), n, b, st, None if z is None else K._ptr(z), None if o is None else K._ptr(o))
    assert ee() == K.KZG_OK
    assert ee(n=6) == INV and ee(n=0) == INV and ee(n=1 << 23) == INV
    assert ee(e=None) == INV and ee(z=None) == INV and ee(o=None) == INV
    assert ee(st=4) == INV
    assert ee(b=0, e=None, z=None, o=None) == K.KZG_OK
    evb = ev.copy()
    evb[1, 5] = big
    assert ee(e=evb) == INV and b"polynomial 1" in last() and b"value 5" in last()
    zb = z2.copy()
    zb[1] = big
    assert ee(z=zb) == INV and b"polynomial 1" in last()
    assert call()  # the context is still fine
    nosrs = K.Engine(0)
    try:
        assert _status(lambda: nosrs.verify_openings_batch(r.coms, r.idx, zl, yl, r.prf, G2)) == K.KZG_ERR_NO_SRS
        got = nosrs.evaluate_evaluations_batch(ev, z2)  # the evaluation needs no SRS
        assert [v.v for v in got] == [NO.barycentric_eval(K.limbs_to_scalars(ev[b]), 5 + b) for b in range(2)]
    finally:
        nosrs.close()


def test_multi_device_contexts(eng):
    rnd = random.Random(8)
    idx = [t % 2 for t in range(8)]
    r = Records(eng, 40, 2, idx, [rnd.randrange(R) for _ in range(8)], 90)
    ev = _random_images(np.random.default_rng(2), (3, 64))
    zs = [K.Scalar(rnd.randrange(R)) for _ in range(3)]
    want = [v.v for v in eng.evaluate_evaluations_batch(ev, zs)]
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(T.BENCH_SECRET_BE, 128)
        assert r.verify(rep)
        ys = list(r.ys)
        ys[1] = (ys[1] + 1) % R
        assert not r.verify(rep, ys=ys)
        assert [v.v for v in rep.evaluate_evaluations_batch(ev, zs)] == want
    finally:
        rep.close()
    rng = K.Engine(devices=[0, 0])
    try:
        rng.srs_generate(T.BENCH_SECRET_BE, 128)
        assert _status(lambda: r.verify(rng)) == K.KZG_ERR_INVALID_ARG
        assert b"range-split" in K.load_library().kzg_last_error(rng._h)
    finally:
        rng.close()


# ---- 7. polynomials in evaluation form -----------------------------------------------------------------------------------
def test_verify_evaluations(eng):
    rnd = random.Random(9)
    n, batch = 4096, 64
    evals = _random_images(np.random.default_rng(3), (batch, n))
    w = NO.domain_root(12)
    zs = [rnd.randrange(R) for _ in range(batch)]
    zs[11] = pow(w, 1234, R)  # one point inside the domain
    coms, prfs, ys = [], [], []
    for b in range(batch):
        coeffs = eng.intt_limbs(evals[b])
        y = eng.evaluate_limbs(coeffs, K.Scalar(zs[b]))
        ys.append(y.v)
        coms.append(eng.commit_evaluations_limbs(evals[b]).p1)
        prfs.append(eng.open_evaluations_limbs(evals[b], K.Scalar(zs[b]), y).p1)
    assert ys[11] == _scalar(evals[11, 1234])
    zsc = [K.Scalar(z) for z in zs]
    ok, got = eng.verify_evaluations_batch(evals, coms, zsc, prfs, G2)
    assert ok and [v.v for v in got] == ys
    ok, got = eng.verify_evaluations_batch(evals, coms, zsc, prfs, G2, want_ys=False)
    assert ok and got is None
    bad = evals.copy()
    bad[40, 77] = _limbs(_scalar(bad[40, 77]) + 1)
    ok, got = eng.verify_evaluations_batch(bad, coms, zsc, prfs, G2)
    assert not ok and [v.v for v in got[:40]] == ys[:40] and got[40].v != ys[40]
    ok, _ = eng.verify_evaluations_batch(evals[:0], [], [], [], G2)
    assert ok


def test_verify_evaluations_in_chunks_with_a_stride(eng):
    """more values than one pass stages (2^22), polynomials a stride apart: 1030 blobs of 4096 values, eight distinct ones"""
    rnd = random.Random(11)
    n, batch, distinct, stride = 4096, 1030, 8, 4096 + 3
    base = _random_images(np.random.default_rng(4), (distinct, n))
    zs8 = [rnd.randrange(R) for _ in range(distinct)]
    coms8, prfs8, ys8 = [], [], []
    for b in range(distinct):
        y = eng.evaluate_limbs(eng.intt_limbs(base[b]), K.Scalar(zs8[b]))
        ys8.append(y.v)
        coms8.append(eng.commit_evaluations_limbs(base[b]).p1)
        prfs8.append(eng.open_evaluations_limbs(base[b], K.Scalar(zs8[b]), y).p1)
    pick = np.arange(batch) % distinct
    buf = np.zeros((batch, stride, 4), dtype=np.uint64)
    buf[:, :n] = base[pick]
    buf[:, n:] = np.uint64(0xFFFFFFFFFFFFFFFF)  # the gaps are never read (they would fail the range check)
    coms = np.ascontiguousarray(np.stack(coms8)[pick])
    prfs = np.ascontiguousarray(np.stack(prfs8)[pick])
    zl = np.ascontiguousarray(np.stack([_limbs(z) for z in zs8])[pick])
    g2 = np.stack(G2)
    lib = K.load_library()
    out = np.zeros((batch, 4), dtype=np.uint64)
    ok = K.C.c_int(0)
    call = lambda e=eng, ev=buf: lib.kzg_verify_evaluations_batch(  # noqa: E731
        e._h, K._ptr(ev), n, batch, stride, K._ptr(coms), K._ptr(zl), K._ptr(prfs), K._ptr(g2), 288, K._ptr(out), K.C.byref(ok))
    assert call() == K.KZG_OK and ok.value == 1
    assert K.limbs_to_scalars(out) == [ys8[b % distinct] for b in range(batch)]
    out2 = np.zeros((batch, 4), dtype=np.uint64)
    assert lib.kzg_evaluate_evaluations_batch(eng._h, K._ptr(buf), n, batch, stride, K._ptr(zl), K._ptr(out2)) == K.KZG_OK
    assert np.array_equal(out, out2)
    bad = buf.copy()
    bad[1027, 9] = _limbs(_scalar(bad[1027, 9]) + 1)  # in the second chunk
    assert call(ev=bad) == K.KZG_OK and ok.value == 0
    assert K.limbs_to_scalars(out[:1027]) == [ys8[b % distinct] for b in range(1027)] and _scalar(out[1027]) != ys8[1027 % distinct]


def test_evaluation_of_large_strided_batches_and_the_largest_domain(eng):
    rnd = random.Random(12)
    lib = K.load_library()
    # five polynomials of 2^20 values, a stride of n + 3: two chunks, the second copied row by row
    n, batch, stride = 1 << 20, 5, (1 << 20) + 3
    buf = np.zeros((batch, stride, 4), dtype=np.uint64)
    buf[:, :n] = _random_images(np.random.default_rng(5), (batch, n))
    w = NO.domain_root(20)
    zs = [rnd.randrange(R), pow(w, 77777, R), 0, rnd.randrange(R), pow(w, n - 1, R)]
    zl = np.stack([_limbs(z) for z in zs])
    out = np.zeros((batch, 4), dtype=np.uint64)
    assert lib.kzg_evaluate_evaluations_batch(eng._h, K._ptr(buf), n, batch, stride, K._ptr(zl), K._ptr(out)) == K.KZG_OK
    for b in range(batch):
        ev = np.ascontiguousarray(buf[b, :n])
        assert _scalar(out[b]) == eng.evaluate_limbs(eng.intt_limbs(ev), K.Scalar(zs[b])).v, b
    assert _scalar(out[1]) == _scalar(buf[1, 77777]) and _scalar(out[4]) == _scalar(buf[4, n - 1])
    # n = 2^22: 4096 tiles, the most partials a lane of the finishing kernel adds
    n = 1 << 22
    ev = _random_images(np.random.default_rng(6), (1, n))
    coeffs = eng.intt_limbs(ev[0])
    w = NO.domain_root(22)
    for z in (rnd.randrange(R), 0, pow(w, n - 5, R), (pow(w, 12345, R) + 1) % R):
        got = eng.evaluate_evaluations_batch(ev, [K.Scalar(z)])
        assert got[0].v == eng.evaluate_limbs(coeffs, K.Scalar(z)).v, z
    top = np.broadcast_to(_limbs(R - 1), ev.shape).copy()
    assert eng.evaluate_evaluations_batch(top, [K.Scalar(rnd.randrange(R))])[0].v == R - 1


def test_errors_of_the_evaluation_form_verifier_and_the_hook(eng):
    rnd = random.Random(13)
    lib = K.load_library()
    last = lambda e=eng: lib.kzg_last_error(e._h)  # noqa: E731
    INV = K.KZG_ERR_INVALID_ARG
    n, batch = 16, 3
    ev = _random_images(np.random.default_rng(7), (batch, n))
    zs = [rnd.randrange(R) for _ in range(batch)]
    zl = np.stack([_limbs(z) for z in zs])
    ys = eng.evaluate_evaluations_batch(ev, zl)
    yl = np.stack([y.limbs() for y in ys])
    coms = np.stack([eng.commit_evaluations_limbs(ev[b]).p1 for b in range(batch)])
    prfs = np.stack([eng.open_evaluations_limbs(ev[b], K.Scalar(zs[b]), ys[b]).p1 for b in range(batch)])
    g2 = np.stack(G2)
    idx = np.arange(batch, dtype=np.uint32)
    out = np.zeros((batch, 4), dtype=np.uint64)
    ok = K.C.c_int(0)
    p = lambda x: None if x is None else K._ptr(x)  # noqa: E731

    def ve(e=eng, ev=ev, n=n, b=batch, st=n, c=coms, z=zl, pf=prfs, g=g2, o=out, v=True):
        return lib.kzg_verify_evaluations_batch(e._h, p(ev), n, b, st, p(c), p(z), p(pf), p(g), 288, p(o), K.C.byref(ok) if v else None)

    assert ve() == K.KZG_OK and ok.value == 1 and K.limbs_to_scalars(out) == [y.v for y in ys]
    assert ve(o=None) == K.KZG_OK and ok.value == 1  # out_ys may be NULL
    for kw in ({"ev": None}, {"c": None}, {"z": None}, {"pf": None}, {"g": None}, {"v": False}):
        assert ve(**kw) == INV, kw
    assert ve(n=12) == INV and ve(st=8) == INV
    big = np.array([0xFFFFFFFFFFFFFFFF] * 4, dtype=np.uint64)
    evb = ev.copy()
    evb[2, 3] = big
    assert ve(ev=evb) == INV and b"polynomial 2" in last() and b"value 3" in last()
    zb = zl.copy()
    zb[1] = big
    assert ve(z=zb) == INV and b"polynomial 1" in last()
    off = prfs.copy()
    off[1, 6] ^= np.uint64(1)
    assert ve(pf=off) == INV and b"record 1" in last() and b"curve" in last()
    assert ve(b=0, ev=None, c=None, z=None, pf=None, g=None) == K.KZG_OK and ok.value == 1
    # the hook: its own pointers
    w = np.stack([_limbs(rnd.randrange(R)) for _ in range(batch)])
    lhs, rhs = np.zeros(18, dtype=np.uint64), np.zeros(18, dtype=np.uint64)

    def lc(e=eng, c=coms, i=idx, z=zl, y=yl, pf=prfs, g=g2, wt=w, l=lhs, r=rhs, v=True):
        return lib.kzg_verify_openings_lincomb(e._h, p(c), batch, p(i), p(z), p(y), p(pf), batch, p(g), 288, p(wt), p(l), p(r),
                                               K.C.byref(ok) if v else None)

    assert lc() == K.KZG_OK and ok.value == 1
    for kw in ({"c": None}, {"i": None}, {"z": None}, {"y": None}, {"pf": None}, {"g": None}, {"wt": None}, {"l": None},
               {"r": None}, {"v": False}):
        assert lc(**kw) == INV, kw
    wb = w.copy()
    wb[2] = big
    assert lc(wt=wb) == INV and b"weight 2" in last()
    # multi-device contexts: a replicated one gives the single device's answers and names what its device found; a
    # range-split one refuses the verifiers and evaluates on its first device
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(T.BENCH_SECRET_BE, 64)
        assert ve(e=rep) == K.KZG_OK and ok.value == 1
        assert lc(e=rep) == K.KZG_OK and ok.value == 1
        assert ve(e=rep, ev=evb) == INV and b"polynomial 2" in last(rep)
        assert lc(e=rep, pf=off) == INV and b"record 1" in last(rep)
    finally:
        rep.close()
    split = K.Engine(devices=[0, 0])
    try:
        split.srs_generate(T.BENCH_SECRET_BE, 64)
        assert ve(e=split) == INV and b"range-split" in last(split)
        assert lc(e=split) == INV and b"range-split" in last(split)
        assert [v.v for v in split.evaluate_evaluations_batch(ev, zl)] == [y.v for y in ys]
    finally:
        split.close()


# ---- 8. concurrency ------------------------------------------------------------------------------------------------------
def test_verify_beside_commitments(eng):
    rnd = random.Random(10)
    idx = [t % 4 for t in range(32)]
    r = Records(eng, 100, 4, idx, [rnd.randrange(R) for _ in range(32)], 95)
    other = K.scalars_to_limbs([rnd.randrange(R) for _ in range(500)])
    want_cm = eng.commit_limbs(other).compress()
    ys_bad = list(r.ys)
    ys_bad[13] = (ys_bad[13] + 1) % R
    errors = []

    def verify():
        try:
            for i in range(4):
                assert r.verify(eng, ys=ys_bad if i & 1 else None) == (not i & 1)
        except Exception as ex:  # noqa: BLE001 -- reported below
            errors.append(ex)

    def commit():
        try:
            for _ in range(8):
                assert eng.commit_limbs(other).compress() == want_cm
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    threads = [threading.Thread(target=f) for f in (verify, verify, commit, commit)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
