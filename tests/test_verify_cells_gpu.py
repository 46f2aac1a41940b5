"""GPU: kzg_verify_cells_batch / kzg_verify_cells_lincomb on cells and proofs from
kzg_cells_and_proofs_fk20 and commitments from kzg_commit: acceptance across shapes and record layouts, rejection of each
corruption, agreement with kzg_verify_points, the two sides against the big-integer restatement, errors, multi-device
contexts, concurrency and the all-same-id skew at the cap."""
import random
import threading
import time

import numpy as np
import pytest

import bigint_twin as T
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import verify_cells_oracle as VO

pytestmark = pytest.mark.gpu
R = K.R_MODULUS
G2 = [K.srs_g2_at(T.BENCH_SECRET_BE, i) for i in range(65)]


def _poly(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R) for _ in range(n)]


class Batch:
    """every cell of `batch` polynomials of n coefficients as records (b, j), in (b, j) order"""

    def __init__(self, e, n, K_, t, batch, seed):
        self.K, self.t = K_, t
        c = np.stack([K.scalars_to_limbs(_poly(n, seed + b)) for b in range(batch)])
        cells, proofs = e.cells_and_proofs_fk20(c, K_, t)
        M, l = (1 << K_) >> t, 1 << t
        self.coms = np.stack([e.commit_limbs(c[b]).p1 for b in range(batch)])
        self.idx = np.repeat(np.arange(batch, dtype=np.uint32), M)
        self.ids = np.tile(np.arange(M, dtype=np.uint32), batch)
        self.vals = np.ascontiguousarray(cells.reshape(batch * M, l, 4))
        self.prf = np.stack([p.p1 for b in range(batch) for p in proofs[b]])

    def pick(self, rows):
        rows = np.asarray(rows, dtype=np.int64)
        return self.idx[rows].copy(), self.ids[rows].copy(), self.vals[rows].copy(), self.prf[rows].copy()

    def verify(self, e, rows=None, coms=None, idx=None, ids=None, vals=None, prf=None):
        ri, rj, rv, rp = self.pick(range(len(self.ids)) if rows is None else rows)
        return e.verify_cells_batch(self.coms if coms is None else coms, ri if idx is None else idx, rj if ids is None else ids,
                                    rv if vals is None else vals, rp if prf is None else prf, self.K, self.t, G2)


@pytest.fixture(scope="module")
def das():
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(4096)
    yield e
    e.close()


@pytest.fixture(scope="module")
def small():
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(256)
    yield e
    e.close()


# ---- acceptance ----------------------------------------------------------------------------------------------------------
def test_das_shape_all_cells_of_eight_polynomials(das):
    b = Batch(das, 4096, 13, 6, 8, 100)
    assert len(b.ids) == 1024
    assert b.verify(das)
    rows = list(range(1024))
    random.Random(1).shuffle(rows)
    assert b.verify(das, rows=rows)
    # one value changed
    ri, rj, rv, rp = b.pick(range(1024))
    rv[517, 3] = K.scalars_to_limbs([(K.limbs_to_scalars(rv[517, 3])[0] + 1) % R])[0]
    assert not b.verify(das, vals=rv)


@pytest.mark.parametrize("t", range(7))
def test_small_shapes_every_cell_size(small, t):
    K_ = min(t + 3, 8)
    n = min(200, 1 << K_)
    b = Batch(small, n, K_, t, 2, 200 + t)
    assert b.verify(small)
    rows = list(range(len(b.ids)))
    random.Random(t).shuffle(rows)
    assert b.verify(small, rows=rows + rows[:5])  # shuffled, with duplicates
    assert b.verify(small, rows=[rows[0]])  # a single record
    ri, rj, rv, rp = b.pick(rows)
    rv[0, 0] = K.scalars_to_limbs([(K.limbs_to_scalars(rv[0, 0])[0] + 5) % R])[0]
    assert not b.verify(small, rows=rows, vals=rv)


def test_empty_batch_infinity_proofs_and_commitment(small):
    assert small.verify_cells_batch([], [], [], np.zeros((0, 4, 4), np.uint64), [], 5, 2, G2)
    lhs, rhs, ok = small.verify_cells_lincomb([], [], [], np.zeros((0, 4, 4), np.uint64), [], 5, 2, G2, [])
    assert ok and not lhs.p1.any() and not rhs.p1.any()
    short = Batch(small, 4, 5, 2, 2, 300)  # n' <= l: every proof is infinity
    assert not short.prf.any()
    assert short.verify(small)
    zero = Batch(small, 1, 5, 2, 1, 301)  # the zero polynomial: infinity commitment, zero values, infinity proofs
    zero.vals[:] = 0
    zero.coms[:] = 0
    assert zero.verify(small)
    zero.vals[3, 1] = K.scalars_to_limbs([1])[0]
    assert not zero.verify(small)


# ---- rejection of each corruption -----------------------------------------------------------------------------------------
def test_each_corruption_is_rejected(small):
    b = Batch(small, 150, 8, 3, 3, 400)
    k = len(b.ids)
    ri, rj, rv, rp = b.pick(range(k))
    assert b.verify(small)
    p2 = rp.copy()
    p2[[4, 9]] = p2[[9, 4]]
    assert not b.verify(small, prf=p2)  # two proofs swapped
    i2 = ri.copy()
    i2[40] = (i2[40] + 1) % 3
    assert not b.verify(small, idx=i2)  # a record pointed at another commitment
    j2 = rj.copy()
    j2[7] = (j2[7] + 1) % 32
    assert not b.verify(small, ids=j2)  # a cell id changed
    p3 = rp.copy()
    shifted = T.g1_add(T.g1_from_blst_p1_limbs([int(x) for x in p3[11]]), T.G1)
    p3[11] = np.array(T.g1_to_blst_p1_limbs(shifted, 3), dtype=np.uint64)
    assert not b.verify(small, prf=p3)  # a proof shifted by G
    c2 = b.coms.copy()
    c2[1] = np.array(T.g1_to_blst_p1_limbs(T.g1_add(T.g1_from_blst_p1_limbs([int(x) for x in c2[1]]), T.G1)), dtype=np.uint64)
    assert not b.verify(small, coms=c2)  # a commitment shifted by G


def test_agrees_with_verify_points(small):
    K_, t = 6, 2
    b = Batch(small, 40, K_, t, 1, 500)
    g1 = np.stack([np.array(T.g1_to_blst_p1_limbs(p), dtype=np.uint64) for p in T.srs_g1(T.BENCH_SECRET_BE, 4)])
    w = NO.domain_root(K_)
    M = 16
    for j in (0, 5, 15):
        for bad in (False, True):
            ri, rj, rv, rp = b.pick([j])
            if bad:
                rv[0, 2] = K.scalars_to_limbs([(K.limbs_to_scalars(rv[0, 2])[0] + 1) % R])[0]
            zs = [K.Scalar(pow(w, j + M * i, R)) for i in range(4)]
            ys = [K.Scalar(v) for v in K.limbs_to_scalars(rv[0])]
            single = K.verify_points(K.G1Point(b.coms[0]), K.G1Point(rp[0]), zs, ys, g1, G2[:5])
            batch = b.verify(small, rows=[j], vals=rv)
            assert single == batch == (not bad)


def test_lincomb_matches_oracle(small):
    K_, t = 5, 2
    b = Batch(small, 20, K_, t, 2, 600)
    rows = [3, 0, 9, 9, 12, 7]
    ri, rj, rv, rp = b.pick(rows)
    rnd = random.Random(6)
    weights = [rnd.randrange(R) for _ in rows]
    lhs, rhs, ok = small.verify_cells_lincomb(b.coms, ri, rj, rv, rp, K_, t, G2, [K.Scalar(x) for x in weights])
    assert ok
    pt = lambda a: T.g1_from_blst_p1_limbs([int(x) for x in a])  # noqa: E731
    vals = [K.limbs_to_scalars(v) for v in rv]
    want_l, want_r = VO.g1_sides(K_, t, [pt(c) for c in b.coms], [int(x) for x in ri], [int(x) for x in rj], vals, [pt(p) for p in rp], weights,
                                 T.srs_g1(T.BENCH_SECRET_BE, 4))
    assert lhs.compress() == T.g1_compress(want_l) and rhs.compress() == T.g1_compress(want_r)
    assert np.array_equal(lhs.p1, np.array(T.g1_to_blst_p1_limbs(want_l), dtype=np.uint64))
    assert np.array_equal(rhs.p1, np.array(T.g1_to_blst_p1_limbs(want_r), dtype=np.uint64))


# ---- errors ---------------------------------------------------------------------------------------------------------------
def _non_g1_point(seed):
    rnd = random.Random(seed)
    while True:
        x = rnd.randrange(T.P)
        y2 = (x * x * x + 4) % T.P
        if pow(y2, (T.P - 1) // 2, T.P) == 1:
            pt = (x, pow(y2, (T.P + 1) // 4, T.P))
            assert not VO.g1_in_subgroup(pt)
            return np.array(T.g1_to_blst_p1_limbs(pt, 5), dtype=np.uint64)


def _status(fn):
    with pytest.raises(K.KzgError) as ei:
        fn()
    return ei.value.status


def test_errors(small):
    b = Batch(small, 30, 5, 2, 2, 700)
    ri, rj, rv, rp = b.pick(range(len(b.ids)))
    lib = K.load_library()
    last = lambda: lib.kzg_last_error(small._h)  # noqa: E731
    call = lambda coms=b.coms, idx=ri, ids=rj, vals=rv, prf=rp, Kd=5, t=2: small.verify_cells_batch(  # noqa: E731
        coms, idx, ids, vals, prf, Kd, t, G2)
    off = rp.copy()
    off[6, 6] ^= np.uint64(1)  # y changed: off the curve
    assert _status(lambda: call(prf=off)) == K.KZG_ERR_INVALID_ARG and b"record 6" in last() and b"curve" in last()
    ng = rp.copy()
    ng[13] = _non_g1_point(1)
    assert _status(lambda: call(prf=ng)) == K.KZG_ERR_INVALID_ARG and b"record 13" in last() and b"not in G1" in last()
    cg = b.coms.copy()
    cg[1] = _non_g1_point(2)
    assert _status(lambda: call(coms=cg)) == K.KZG_ERR_INVALID_ARG and b"commitment 1" in last() and b"not in G1" in last()
    big = rv.copy()
    big[2, 1] = np.array([0xFFFFFFFFFFFFFFFF] * 4, dtype=np.uint64)
    assert _status(lambda: call(vals=big)) == K.KZG_ERR_INVALID_ARG and b"record 2" in last()
    bad_idx = ri.copy()
    bad_idx[0] = 2
    assert _status(lambda: call(idx=bad_idx)) == K.KZG_ERR_INVALID_ARG
    bad_id = rj.copy()
    bad_id[0] = 8
    assert _status(lambda: call(ids=bad_id)) == K.KZG_ERR_INVALID_ARG
    assert _status(lambda: call(Kd=23)) == K.KZG_ERR_INVALID_ARG
    assert _status(lambda: call(t=6, vals=np.zeros((len(rj), 64, 4), np.uint64))) == K.KZG_ERR_INVALID_ARG
    g2_bad = [g.copy() for g in G2[:5]]
    g2_bad[4][3] ^= np.uint64(1)
    assert _status(lambda: small.verify_cells_batch(b.coms, ri, rj, rv, rp, 5, 2, g2_bad)) == K.KZG_ERR_INVALID_ARG
    assert b.verify(small)  # the context is still fine
    nosrs = K.Engine(0)
    try:
        assert _status(lambda: nosrs.verify_cells_batch(b.coms, ri, rj, rv, rp, 5, 2, G2)) == K.KZG_ERR_NO_SRS
    finally:
        nosrs.close()
    short = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(3)
    try:
        assert _status(lambda: short.verify_cells_batch(b.coms, ri, rj, rv, rp, 5, 2, G2)) == K.KZG_ERR_NO_SRS
    finally:
        short.close()


# ---- multi-device, concurrency, skew --------------------------------------------------------------------------------------
def test_multi_device_contexts(small):
    b = Batch(small, 100, 7, 3, 2, 800)
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(T.BENCH_SECRET_BE, 128)
        assert b.verify(rep)
        ri, rj, rv, rp = b.pick(range(len(b.ids)))
        rp[[1, 2]] = rp[[2, 1]]
        assert not b.verify(rep, prf=rp)
    finally:
        rep.close()
    rng = K.Engine(devices=[0, 0])
    try:
        rng.srs_generate(T.BENCH_SECRET_BE, 128)
        assert _status(lambda: b.verify(rng)) == K.KZG_ERR_INVALID_ARG
        assert b"range-split" in K.load_library().kzg_last_error(rng._h)
    finally:
        rng.close()


def test_verify_beside_commitments(small):
    b = Batch(small, 120, 8, 4, 2, 900)
    other = K.scalars_to_limbs(_poly(200, 5))
    want_cm = small.commit_limbs(other).compress()
    ri, rj, rv, rp = b.pick(range(len(b.ids)))
    rv_bad = rv.copy()
    rv_bad[3, 3] = rv_bad[4, 3]
    errors, stop = [], threading.Event()

    def verify():
        try:
            for i in range(4):
                assert b.verify(small, vals=rv_bad if i & 1 else rv) == (not i & 1)
        except Exception as ex:  # noqa: BLE001 -- reported below
            errors.append(ex)

    def commit_loop():
        try:
            while not stop.is_set():
                assert small.commit_limbs(other).compress() == want_cm
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    cl = threading.Thread(target=commit_loop)
    cl.start()
    vt = threading.Thread(target=verify)
    vt.start()
    vt.join()
    stop.set()
    cl.join()
    assert not errors, errors


def test_all_same_cell_id_at_the_cap(small):
    b = Batch(small, 64, 6, 0, 1, 1000)  # l = 1, M = 64
    cap = 1 << 20
    rows = np.full(cap, 17)
    t0 = time.perf_counter()
    assert b.verify(small, rows=rows)
    dt = time.perf_counter() - t0
    ri, rj, rv, rp = b.pick(rows)
    rv[cap - 1, 0] = K.scalars_to_limbs([(K.limbs_to_scalars(rv[cap - 1, 0])[0] + 1) % R])[0]
    assert not b.verify(small, rows=rows, vals=rv)
    spread = np.arange(cap) % 64  # the same number of records over every id
    t1 = time.perf_counter()
    assert b.verify(small, rows=spread)
    dt_spread = time.perf_counter() - t1
    assert dt < 4 * dt_spread + 1.0, (dt, dt_spread)
    with pytest.raises(K.KzgError) as ei:
        b.verify(small, rows=np.full(cap + 1, 17))
    assert ei.value.status == K.KZG_ERR_INVALID_ARG
