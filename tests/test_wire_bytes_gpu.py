"""GPU: the verifiers on inputs as they travel -- kzg_g1_uncompress_batch and
kzg_fr_from_bytes_batch against kzg_g1_uncompress and the big-integer oracle, every rejection class planted at known indices;
the _lincomb_bytes hooks against the existing hooks on the host-decoded inputs, bit for bit, in both orders; each single
corruption caught and named; kzg_verify_blobs_batch_bytes against kzg_verify_evaluations_batch; multi-device contexts and
threads.  References: oracle/bigint_twin.py, oracle_ctypes (p1_compress), tests/cells_oracle.py, tests/trapdoor_oracle.py,
tests/wire_oracle.py and the existing uncompressed entry points."""
import random
import threading

import numpy as np
import pytest

import bigint_twin as T
import kzg_poly_commit_exploration_amd as K
import oracle_ctypes as O
import trapdoor_oracle as TO
import wire_oracle as W

pytestmark = pytest.mark.gpu
R = K.R_MODULUS
G2 = [K.srs_g2_at(T.BENCH_SECRET_BE, i) for i in range(65)]
INV = K.KZG_ERR_INVALID_ARG
NAT, BRP = K.KZG_ORDER_NATURAL, K.KZG_ORDER_BIT_REVERSED
SIZES = (0, 1, 63, 64, 65, 4097)


@pytest.fixture(scope="module")
def eng():
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(4096)
    yield e
    e.close()


@pytest.fixture(scope="module")
def torsion():
    return TO.torsion_points()


def last(e):
    return K.load_library().kzg_last_error(e._h)


def fails(fn):
    with pytest.raises(K.KzgError) as ei:
        fn()
    return ei.value


def compress_rows(rows):
    return b"".join(O.p1_compress(r) for r in np.asarray(rows, dtype=np.uint64).reshape(-1, 18))


def host_uncompress(data):
    """today's route: kzg_g1_uncompress per point"""
    return np.stack([K.G1Point.uncompress(data[48 * i:48 * i + 48]).p1 for i in range(len(data) // 48)]) if data else \
        np.zeros((0, 18), dtype=np.uint64)


def host_scalars(data):
    """today's route: big-endian -> blst_fr per value"""
    return K.scalars_to_limbs([int.from_bytes(data[32 * i:32 * i + 32], "big") for i in range(len(data) // 32)])


def plant(data, width, at, item):
    return data[:width * at] + item + data[width * (at + 1):]


# ---- 5. the decoders on their own ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def srs_bytes():
    rows = O.srs_g1(4097, T.BENCH_SECRET_BE)
    return [O.p1_compress(r) for r in rows]


@pytest.mark.parametrize("n", SIZES)
def test_g1_uncompress_batch_equals_the_host_decoder(eng, srs_bytes, n):
    pts = list(srs_bytes[:n])
    inf = T.g1_compress(T.INF)
    for at in (0, n // 2, n - 1):
        if n > 2:
            pts[at] = inf
    for at in range(3, n, 7):
        if pts[at] != inf:
            pts[at] = W.flip_sign(pts[at])
    data = b"".join(pts)
    for check in (False, True):
        got = eng.g1_uncompress_batch(data, check_subgroup=check)
        assert got.shape == (n, 18) and np.array_equal(got, host_uncompress(data).reshape(n, 18)), (n, check)
    if n == 1:
        assert np.array_equal(eng.g1_uncompress_batch(inf)[0], np.zeros(18, dtype=np.uint64))


def test_g1_uncompress_batch_reports_where_it_was_planted(eng, srs_bytes, torsion):
    n = 65
    data = b"".join(srs_bytes[:n])
    for name, enc in W.malformed_points().items():
        for at in (0, 31, n - 1):
            for check in (False, True):
                ex = fails(lambda: eng.g1_uncompress_batch(plant(data, 48, at, enc), check_subgroup=check))
                assert ex.status == INV and ex.bad_index == at, (name, at)
                assert b"point %d " % at in last(eng) and b"not a valid compressed point" in last(eng), (name, last(eng))
    classes = list(W.malformed_points().values())
    two = plant(plant(data, 48, 50, classes[0]), 48, 12, classes[3])
    assert fails(lambda: eng.g1_uncompress_batch(two)).bad_index == 12
    two = plant(plant(data, 48, 7, classes[5]), 48, 64, classes[1])
    assert fails(lambda: eng.g1_uncompress_batch(two, check_subgroup=True)).bad_index == 7
    for q, tp in list(torsion.items()) + [(3, TO.ORDER3[0])]:
        for at in (0, 40, n - 1):
            shifted = plant(data, 48, at, W.plus_torsion(srs_bytes[at], tp))
            ex = fails(lambda: eng.g1_uncompress_batch(shifted, check_subgroup=True))
            assert ex.status == INV and ex.bad_index == at and b"not in G1" in last(eng), (q, at)
            got = eng.g1_uncompress_batch(shifted)  # without the check it is a point of the curve like any other
            assert np.array_equal(got, host_uncompress(shifted)), (q, at)
    # a torsion point behind a malformed one, and in front of it: the lesser index
    mixed = plant(plant(data, 48, 9, classes[0]), 48, 30, W.plus_torsion(srs_bytes[30], torsion[11]))
    assert fails(lambda: eng.g1_uncompress_batch(mixed, check_subgroup=True)).bad_index == 9
    mixed = plant(plant(data, 48, 33, classes[0]), 48, 30, W.plus_torsion(srs_bytes[30], torsion[11]))
    assert fails(lambda: eng.g1_uncompress_batch(mixed, check_subgroup=True)).bad_index == 30
    assert np.array_equal(eng.g1_uncompress_batch(data), host_uncompress(data))  # the context is still fine


@pytest.mark.parametrize("n", SIZES)
def test_fr_from_bytes_batch(eng, n):
    rnd = random.Random(n)
    vals = ([0, 1, R - 1] + [rnd.randrange(R) for _ in range(n)])[:n]
    data = b"".join(W.fr_be_raw(v) for v in vals)
    got = eng.fr_from_bytes_batch(data)
    assert got.shape == (n, 4)
    assert [[int(x) for x in row] for row in got] == [T.fr_to_mont_limbs(v) for v in vals]
    if n < 3:
        return
    for v in W.FR_REJECTED:
        for at in (0, n // 2, n - 1):
            ex = fails(lambda: eng.fr_from_bytes_batch(plant(data, 32, at, W.fr_be_raw(v))))
            assert ex.status == INV and ex.bad_index == at and b"value %d " % at in last(eng) and b"not below r" in last(eng)
    two = plant(plant(data, 32, n - 2, W.fr_be_raw(R)), 32, 1, W.fr_be_raw(R + 1))
    assert fails(lambda: eng.fr_from_bytes_batch(two)).bad_index == 1


# ---- records ---------------------------------------------------------------------------------------------------------------
class Cells:
    """`rows` of the cells of `batch` polynomials of n coefficients as wire records, with the host-decoded inputs beside them"""

    def __init__(self, e, n, K_, t, batch, rows, seed):
        rnd = random.Random(seed)
        self.K, self.t = K_, t
        M, l = (1 << K_) >> t, 1 << t
        c = np.stack([K.scalars_to_limbs([rnd.randrange(R) for _ in range(n)]) for _ in range(batch)])
        cells, proofs = e.cells_and_proofs_fk20(c, K_, t)
        cells = cells.reshape(batch, M, l, 4)
        self.idx = np.array([b for b, j in rows], dtype=np.uint32)
        self.ids = np.array([j for b, j in rows], dtype=np.uint32)
        self.ints = [K.limbs_to_scalars(cells[b, j]) for b, j in rows]  # natural order, this API's cell ids
        self.coms48 = compress_rows([e.commit_limbs(c[b]).p1 for b in range(batch)])
        self.prf48 = compress_rows([proofs[b][j].p1 for b, j in rows])
        self.cells_be = b"".join(W.fr_list_be(r) for r in self.ints)
        sids, srows = W.cells_to_spec(self.ids, self.ints, K_, t)  # the same data as the sampling specs order it
        self.spec_ids = np.array(sids, dtype=np.uint32)
        self.spec_be = b"".join(W.fr_list_be(r) for r in srows)
        self.weights = [K.Scalar(rnd.randrange(R)) for _ in rows]

    def wire(self, order=NAT, **kw):
        a = dict(coms=self.coms48, idx=self.idx, ids=self.ids if order == NAT else self.spec_ids,
                 cells=self.cells_be if order == NAT else self.spec_be, prf=self.prf48)
        a.update(kw)
        return a["coms"], a["idx"], a["ids"], a["cells"], a["prf"], self.K, self.t, G2

    def decoded(self):
        return (host_uncompress(self.coms48), self.idx, self.ids, host_scalars(self.cells_be).reshape(len(self.ids), -1, 4),
                host_uncompress(self.prf48), self.K, self.t, G2)


def _das_rows(rnd, batch, M, count):
    return [(t % batch, rnd.randrange(M)) for t in range(count)]


CELL_SHAPES = {
    "das": lambda rnd: (4096, 13, 6, 4, _das_rows(rnd, 4, 128, 128)),
    "points": lambda rnd: (200, 8, 0, 2, [(b, j) for b in range(2) for j in range(0, 256, 5)]),
    "one cell, infinity proofs": lambda rnd: (64, 6, 6, 3, [(0, 0), (1, 0), (2, 0)]),
    "constants": lambda rnd: (1, 5, 2, 2, [(b, j) for b in range(2) for j in range(8)]),
    "repeats": lambda rnd: (100, 7, 2, 3, [(0, 5), (1, 5), (2, 5), (0, 5), (0, 5), (1, 9), (1, 9), (2, 31), (0, 0)]),
}


@pytest.mark.parametrize("shape", sorted(CELL_SHAPES))
def test_cells_bytes_give_the_same_sides(eng, shape):
    n, K_, t, batch, rows = CELL_SHAPES[shape](random.Random(len(shape)))
    c = Cells(eng, n, K_, t, batch, rows, 500 + len(shape))
    if shape in ("one cell, infinity proofs", "constants"):
        assert c.prf48 == T.g1_compress(T.INF) * len(rows)
    want_l, want_r, want_ok = eng.verify_cells_lincomb(*c.decoded(), c.weights)
    assert want_ok
    for order in (NAT, BRP):
        lhs, rhs, ok = eng.verify_cells_lincomb_bytes(*c.wire(order), c.weights, order=order)
        assert ok and np.array_equal(lhs.p1, want_l.p1) and np.array_equal(rhs.p1, want_r.p1), (shape, order)
        assert eng.verify_cells_batch_bytes(*c.wire(order), order=order)
    if t:  # the orders differ: natural bytes read as bit-reversed are other cells
        assert not eng.verify_cells_batch_bytes(*c.wire(NAT), order=BRP) or shape == "constants"
    assert eng.verify_cells_batch_bytes(b"", [], [], b"", b"", K_, t, G2)  # k = 0
    lhs, rhs, ok = eng.verify_cells_lincomb_bytes(b"", [], [], b"", b"", K_, t, G2, [])
    assert ok and not lhs.p1.any() and not rhs.p1.any()


class Openings:
    """openings of `polys` random polynomials of n coefficients as wire records: record t = (polynomial idx[t], point zs[t])"""

    def __init__(self, e, n, polys, idx, zs, seed):
        rnd = random.Random(seed)
        coeffs = [[rnd.randrange(R) for _ in range(n)] for _ in range(polys)]
        limbs = [K.scalars_to_limbs(c) for c in coeffs]
        self.idx = np.array(idx, dtype=np.uint32)
        self.zs = [z % R for z in zs]
        self.ys = [TO.poly_eval(coeffs[b], z) for b, z in zip(idx, self.zs)]
        self.coms48 = compress_rows([e.commit_limbs(l).p1 for l in limbs])
        self.prf48 = compress_rows([np.zeros(18, dtype=np.uint64) if n == 1 else
                                    e.open_limbs(limbs[b], K.Scalar(z), K.Scalar(y)).p1 for b, z, y in zip(idx, self.zs, self.ys)])
        self.weights = [K.Scalar(rnd.randrange(R)) for _ in idx]

    def wire(self, **kw):
        a = dict(coms=self.coms48, idx=self.idx, zs=W.fr_list_be(self.zs), ys=W.fr_list_be(self.ys), prf=self.prf48)
        a.update(kw)
        return a["coms"], a["idx"], a["zs"], a["ys"], a["prf"], G2[:2]

    def decoded(self):
        return (host_uncompress(self.coms48), self.idx, host_scalars(W.fr_list_be(self.zs)), host_scalars(W.fr_list_be(self.ys)),
                host_uncompress(self.prf48), G2[:2])


OPENING_SHAPES = {
    "shared points": lambda rnd, z: (20, 5, [t % 5 for t in range(30)], [z if t % 3 else z + 1 for t in range(30)]),
    "distinct points": lambda rnd, z: (33, 2, [t % 2 for t in range(24)], [rnd.randrange(R) for _ in range(24)]),
    "one record": lambda rnd, z: (10, 1, [0], [z]),
    "constants": lambda rnd, z: (1, 2, [0, 1, 1], [z, z, 5]),
}


@pytest.mark.parametrize("shape", sorted(OPENING_SHAPES))
def test_openings_bytes_give_the_same_sides(eng, shape):
    rnd = random.Random(len(shape))
    n, polys, idx, zs = OPENING_SHAPES[shape](rnd, rnd.randrange(R))
    o = Openings(eng, n, polys, idx, zs, 600 + len(shape))
    want_l, want_r, want_ok = eng.verify_openings_lincomb(*o.decoded(), o.weights)
    assert want_ok
    lhs, rhs, ok = eng.verify_openings_lincomb_bytes(*o.wire(), o.weights)
    assert ok and np.array_equal(lhs.p1, want_l.p1) and np.array_equal(rhs.p1, want_r.p1), shape
    assert eng.verify_openings_batch_bytes(*o.wire())
    assert eng.verify_openings_batch_bytes(b"", [], b"", b"", b"", G2[:2])  # k = 0


# ---- 7. each single corruption ---------------------------------------------------------------------------------------------
def _bump(data, at, by=1):
    """the scalar at index `at` of a string of big-endian scalars, plus `by`"""
    v = (int.from_bytes(data[32 * at:32 * at + 32], "big") + by) % R
    return plant(data, 32, at, W.fr_be(v))


def test_cells_each_corruption_is_caught_and_named(eng, torsion):
    K_, t, batch = 8, 3, 3
    rows = [(b, j) for b in range(batch) for j in range(0, 32, 3)]
    c = Cells(eng, 150, K_, t, batch, rows, 700)
    k, l = len(rows), 1 << t
    for order in (NAT, BRP):
        call = lambda **kw: eng.verify_cells_batch_bytes(*c.wire(order, **kw), order=order)  # noqa: E731,B023
        cells = c.cells_be if order == NAT else c.spec_be  # noqa: F841
        assert call()
        assert not call(cells=_bump(cells, 13 * l + 5))  # one value changed by one
        assert not call(prf=plant(c.prf48, 48, 9, W.flip_sign(c.prf48[48 * 9:48 * 10])))  # -P is a valid point: the check fails
        assert not call(coms=plant(c.coms48, 48, 1, W.flip_sign(c.coms48[48:96])))
        for name, enc in W.malformed_points().items():
            ex = fails(lambda: call(prf=plant(c.prf48, 48, 17, enc)))
            assert ex.status == INV and b"proof of record 17 " in last(eng) and b"not a valid compressed point" in last(eng), name
            ex = fails(lambda: call(coms=plant(c.coms48, 48, 2, enc)))
            assert ex.status == INV and b"commitment 2 " in last(eng) and b"not a valid compressed point" in last(eng), name
        for q, tp in torsion.items():
            ex = fails(lambda: call(prf=plant(c.prf48, 48, 4, W.plus_torsion(c.prf48[48 * 4:48 * 5], tp))))
            assert ex.status == INV and b"proof of record 4 " in last(eng) and b"not in G1" in last(eng), q
            ex = fails(lambda: call(coms=plant(c.coms48, 48, 0, W.plus_torsion(c.coms48[:48], tp))))
            assert ex.status == INV and b"commitment 0 " in last(eng) and b"not in G1" in last(eng), q
        for v in W.FR_REJECTED:
            ex = fails(lambda: call(cells=plant(cells, 32, 20 * l + 6, W.fr_be_raw(v))))
            assert ex.status == INV and b"record 20: value 6 " in last(eng) and b"not below r" in last(eng), v
        assert call()
    # arguments: the order, and what the sibling rejects before it reads a point or a value
    ex = fails(lambda: eng.verify_cells_batch_bytes(*c.wire(), order=2))
    assert ex.status == INV and b"order" in last(eng)
    ids = c.ids.copy()
    ids[3] = 32
    assert fails(lambda: eng.verify_cells_batch_bytes(*c.wire(ids=ids))).status == INV and b"record 3" in last(eng)
    idx = c.idx.copy()
    idx[5] = batch
    assert fails(lambda: eng.verify_cells_batch_bytes(*c.wire(idx=idx))).status == INV and b"record 5" in last(eng)
    wide = c.wire(cells=bytes(32 * (k << 7)))  # log_cell = 7: no such cell size
    assert fails(lambda: eng.verify_cells_batch_bytes(*wide[:5], 8, 7, G2)).status == INV and b"shape" in last(eng)
    lib = K.load_library()
    ok = K.C.c_int(0)
    keep = [np.frombuffer(x, dtype=np.uint8) for x in (c.coms48, c.cells_be, c.prf48)] + [np.stack(G2)]
    null = lambda **kw: lib.kzg_verify_cells_batch_bytes(  # noqa: E731
        eng._h, kw.get("c", K._ptr(keep[0])), batch, kw.get("i", K._ptr(c.idx)), kw.get("j", K._ptr(c.ids)),
        kw.get("v", K._ptr(keep[1])), kw.get("p", K._ptr(keep[2])), k, K_, t, NAT, kw.get("g", K._ptr(keep[3])), 288,
        kw.get("o", K.C.byref(ok)))
    assert null() == K.KZG_OK and ok.value == 1
    for name in "cijvpgo":
        assert null(**{name: None}) == INV, name
    nosrs = K.Engine(0)
    try:
        assert fails(lambda: nosrs.verify_cells_batch_bytes(*c.wire())).status == K.KZG_ERR_NO_SRS
        assert np.array_equal(nosrs.g1_uncompress_batch(c.prf48), host_uncompress(c.prf48))  # the decoders need no SRS
        assert np.array_equal(nosrs.fr_from_bytes_batch(c.cells_be), host_scalars(c.cells_be))
    finally:
        nosrs.close()


def test_openings_each_corruption_is_caught_and_named(eng, torsion):
    rnd = random.Random(8)
    o = Openings(eng, 50, 3, [t % 3 for t in range(12)], [rnd.randrange(R) for _ in range(12)], 800)
    call = lambda **kw: eng.verify_openings_batch_bytes(*o.wire(**kw))  # noqa: E731
    zs, ys = W.fr_list_be(o.zs), W.fr_list_be(o.ys)
    assert call()
    assert not call(ys=_bump(ys, 5))
    assert not call(zs=_bump(zs, 6))
    assert not call(prf=plant(o.prf48, 48, 7, W.flip_sign(o.prf48[48 * 7:48 * 8])))
    assert not call(coms=plant(o.coms48, 48, 2, W.flip_sign(o.coms48[96:144])))
    for name, enc in W.malformed_points().items():
        ex = fails(lambda: call(prf=plant(o.prf48, 48, 11, enc)))
        assert ex.status == INV and b"proof of record 11 " in last(eng) and b"not a valid compressed point" in last(eng), name
        ex = fails(lambda: call(coms=plant(o.coms48, 48, 0, enc)))
        assert ex.status == INV and b"commitment 0 " in last(eng) and b"not a valid compressed point" in last(eng), name
    for q, tp in torsion.items():
        ex = fails(lambda: call(prf=plant(o.prf48, 48, 3, W.plus_torsion(o.prf48[48 * 3:48 * 4], tp))))
        assert ex.status == INV and b"proof of record 3 " in last(eng) and b"not in G1" in last(eng), q
        ex = fails(lambda: call(coms=plant(o.coms48, 48, 1, W.plus_torsion(o.coms48[48:96], tp))))
        assert ex.status == INV and b"commitment 1 " in last(eng) and b"not in G1" in last(eng), q
    for v in W.FR_REJECTED:
        ex = fails(lambda: call(ys=plant(ys, 32, 4, W.fr_be_raw(v))))
        assert ex.status == INV and b"record 4: the claimed y " in last(eng) and b"not below r" in last(eng), v
        ex = fails(lambda: call(zs=plant(zs, 32, 8, W.fr_be_raw(v))))
        assert ex.status == INV and b"record 8: the point z " in last(eng) and b"not below r" in last(eng), v
    idx = o.idx.copy()
    idx[0] = 3
    assert fails(lambda: call(idx=idx)).status == INV and b"record 0" in last(eng)
    lib = K.load_library()
    ok = K.C.c_int(0)
    keep = [np.frombuffer(x, dtype=np.uint8) for x in (o.coms48, zs, ys, o.prf48)] + [np.stack(G2[:2])]
    null = lambda **kw: lib.kzg_verify_openings_batch_bytes(  # noqa: E731
        eng._h, kw.get("c", K._ptr(keep[0])), 3, kw.get("i", K._ptr(o.idx)), kw.get("z", K._ptr(keep[1])),
        kw.get("y", K._ptr(keep[2])), kw.get("p", K._ptr(keep[3])), 12, kw.get("g", K._ptr(keep[4])), 288,
        kw.get("o", K.C.byref(ok)))
    assert null() == K.KZG_OK and ok.value == 1
    for name in "cizypgo":
        assert null(**{name: None}) == INV, name
    assert call()


# ---- 8. blobs --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blobs(eng):
    """three distinct blobs per size with their commitments, challenges and proofs (tiled to the batch sizes below)"""
    out = {}
    for n in (1, 64, 4096):
        rnd = random.Random(900 + n)
        vals = [[rnd.randrange(R) for _ in range(n)] for _ in range(3)]
        zs = [rnd.randrange(R) for _ in range(3)]
        if n > 1:
            zs[1] = pow(K.domain_root(n.bit_length() - 1).v, 5 % n, R)  # a point of the domain
        coms, prfs = [], []
        for b in range(3):
            ev = K.scalars_to_limbs(vals[b])
            if n == 1:  # a constant: commit to it as a polynomial; the quotient is zero
                coms.append(eng.commit_limbs(ev).p1)
                prfs.append(np.zeros(18, dtype=np.uint64))
                continue
            y = eng.evaluate_evaluations_batch(ev, [K.Scalar(zs[b])])[0]
            coms.append(eng.commit_evaluations_limbs(ev).p1)
            prfs.append(eng.open_evaluations_limbs(ev, K.Scalar(zs[b]), y).p1)
        out[n] = (vals, zs, [O.p1_compress(c) for c in coms], [O.p1_compress(p) for p in prfs])
    return out


@pytest.mark.parametrize("batch", (1, 3, 64))
@pytest.mark.parametrize("n", (1, 64, 4096))
def test_blobs_bytes_against_the_evaluation_form_verifier(eng, blobs, n, batch):
    vals, zs, coms48, prfs48 = blobs[n]
    pick = [b % 3 for b in range(batch)]
    nat = b"".join(W.fr_list_be(vals[p]) for p in pick)
    spec = b"".join(W.fr_list_be(W.blob_to_spec(vals[p])) for p in pick)
    coms, prfs = b"".join(coms48[p] for p in pick), b"".join(prfs48[p] for p in pick)
    zs_be = W.fr_list_be([zs[p] for p in pick])
    want_ok, want_ys = eng.verify_evaluations_batch(host_scalars(nat).reshape(batch, n, 4), host_uncompress(coms), host_scalars(zs_be),
                                                    host_uncompress(prfs), G2[:2])
    assert want_ok
    want_be = W.fr_list_be([y.v for y in want_ys])
    for order, data in ((NAT, nat), (BRP, spec)):
        ok, ys_be = eng.verify_blobs_batch_bytes(data, n, coms, zs_be, prfs, G2[:2], order=order)
        assert ok and ys_be == want_be, (n, batch, order)
        ok, ys_be = eng.verify_blobs_batch_bytes(data, n, coms, zs_be, prfs, G2[:2], order=order, want_ys=False)
        assert ok and ys_be is None
        b, i = batch - 1, (n * 5) // 7
        ok, ys_be = eng.verify_blobs_batch_bytes(_bump(data, b * n + i), n, coms, zs_be, prfs, G2[:2], order=order)
        assert not ok and ys_be[:32 * b] == want_be[:32 * b] and ys_be[32 * b:] != want_be[32 * b:]
        for v in W.FR_REJECTED:
            ex = fails(lambda: eng.verify_blobs_batch_bytes(plant(data, 32, b * n + i, W.fr_be_raw(v)), n, coms, zs_be, prfs,  # noqa: B023
                                                            G2[:2], order=order))  # noqa: B023
            assert ex.status == INV and b"polynomial %d: value %d " % (b, i) in last(eng) and b"not below r" in last(eng)
    ex = fails(lambda: eng.verify_blobs_batch_bytes(nat, n, coms, plant(zs_be, 32, batch - 1, W.fr_be_raw(R)), prfs, G2[:2]))
    assert ex.status == INV and b"polynomial %d: the point z " % (batch - 1) in last(eng)
    ex = fails(lambda: eng.verify_blobs_batch_bytes(nat, n, plant(coms, 48, 0, W.malformed_points()["x = p"]), zs_be, prfs, G2[:2]))
    assert ex.status == INV and b"commitment 0 " in last(eng) and b"not a valid compressed point" in last(eng)
    assert fails(lambda: eng.verify_blobs_batch_bytes(nat, n, coms, zs_be, prfs, G2[:2], order=7)).status == INV


def test_blobs_in_chunks_with_a_stride(eng, blobs):
    """more values than one pass stages (2^22) and blobs a stride apart: 1030 blobs of 4096 values, three distinct ones"""
    vals, zs, coms48, prfs48 = blobs[4096]
    n, batch, stride = 4096, 1030, 4096 + 3
    one = [np.frombuffer(W.fr_list_be(W.blob_to_spec(v)), dtype=np.uint8).reshape(n, 32) for v in vals]
    buf = np.full((batch, stride, 32), 0xFF, dtype=np.uint8)  # the gaps are never read (they are not below r)
    for b in range(batch):
        buf[b, :n] = one[b % 3]
    keep = [np.frombuffer(b"".join(x[b % 3] for b in range(batch)), dtype=np.uint8) for x in (coms48, prfs48)]
    zl = np.frombuffer(W.fr_list_be([zs[b % 3] for b in range(batch)]), dtype=np.uint8)
    g2 = np.stack(G2[:2])
    out = np.zeros((batch, 32), dtype=np.uint8)
    ok = K.C.c_int(0)
    lib = K.load_library()
    call = lambda data: lib.kzg_verify_blobs_batch_bytes(  # noqa: E731
        eng._h, K._ptr(data), n, batch, stride, BRP, K._ptr(keep[0]), K._ptr(zl), K._ptr(keep[1]), K._ptr(g2), 288, K._ptr(out),
        K.C.byref(ok))
    assert call(buf) == K.KZG_OK and ok.value == 1
    ys3 = [eng.evaluate_evaluations_batch(K.scalars_to_limbs(vals[b]), [K.Scalar(zs[b])])[0].v for b in range(3)]
    assert out.tobytes() == W.fr_list_be([ys3[b % 3] for b in range(batch)])
    bad = buf.copy()
    # in the second chunk; blob 1028 is a copy of blob 2, whose challenge lies outside the domain (blob 1's is a point of the
    # domain, where the value is one of the blob's values and the others do not enter the check)
    bad[1028, 9, 31] ^= 1
    assert call(bad) == K.KZG_OK and ok.value == 0
    assert out[:1028].tobytes() == W.fr_list_be([ys3[b % 3] for b in range(1028)]) and out[1028].tobytes() != W.fr_be(ys3[2])
    bad[1028, 9] = np.frombuffer(W.fr_be_raw(R), dtype=np.uint8)
    assert call(bad) == INV and b"polynomial 1028: value 9 " in last(eng)


# ---- 9. contexts and threads -----------------------------------------------------------------------------------------------
def test_multi_device_contexts(eng, blobs):
    c = Cells(eng, 100, 7, 2, 2, [(b, j) for b in range(2) for j in range(0, 32, 4)], 1000)
    rnd = random.Random(10)
    o = Openings(eng, 40, 2, [t % 2 for t in range(8)], [rnd.randrange(R) for _ in range(8)], 1001)
    vals, zs, coms48, prfs48 = blobs[64]
    blob_args = (b"".join(W.fr_list_be(v) for v in vals), 64, b"".join(coms48), W.fr_list_be(zs), b"".join(prfs48), G2[:2])
    want_ys = eng.verify_blobs_batch_bytes(*blob_args)[1]
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(T.BENCH_SECRET_BE, 128)
        for order in (NAT, BRP):
            assert rep.verify_cells_batch_bytes(*c.wire(order), order=order)
        assert not rep.verify_cells_batch_bytes(*c.wire(cells=_bump(c.cells_be, 7)))
        assert rep.verify_openings_batch_bytes(*o.wire())
        assert not rep.verify_openings_batch_bytes(*o.wire(ys=_bump(W.fr_list_be(o.ys), 1)))
        assert rep.verify_blobs_batch_bytes(*blob_args) == (True, want_ys)
        ex = fails(lambda: rep.verify_cells_batch_bytes(*c.wire(prf=plant(c.prf48, 48, 5, W.malformed_points()["x + p"]))))
        assert ex.status == INV and b"proof of record 5 " in last(rep)
        assert np.array_equal(rep.g1_uncompress_batch(c.prf48, check_subgroup=True), host_uncompress(c.prf48))
        assert np.array_equal(rep.fr_from_bytes_batch(c.cells_be), host_scalars(c.cells_be))
    finally:
        rep.close()
    split = K.Engine(devices=[0, 0])
    try:
        split.srs_generate(T.BENCH_SECRET_BE, 128)
        for fn in (lambda: split.verify_cells_batch_bytes(*c.wire()), lambda: split.verify_openings_batch_bytes(*o.wire()),
                   lambda: split.verify_blobs_batch_bytes(*blob_args)):
            assert fails(fn).status == INV and b"range-split" in last(split)
    finally:
        split.close()


def test_four_threads_verify_bytes_while_a_fifth_commits(eng, blobs):
    rnd = random.Random(11)
    c = Cells(eng, 150, 8, 3, 3, [(b, j) for b in range(3) for j in range(32)], 1100)
    o = Openings(eng, 100, 4, [t % 4 for t in range(32)], [rnd.randrange(R) for _ in range(32)], 1101)
    vals, zs, coms48, prfs48 = blobs[64]
    blob_args = (b"".join(W.fr_list_be(W.blob_to_spec(v)) for v in vals), 64, b"".join(coms48), W.fr_list_be(zs), b"".join(prfs48),
                 G2[:2])
    bad_cells, bad_ys = _bump(c.spec_be, 100), _bump(W.fr_list_be(o.ys), 13)
    other = K.scalars_to_limbs([rnd.randrange(R) for _ in range(500)])
    want_cm = eng.commit_limbs(other).compress()
    errors = []

    def guarded(fn):
        def run():
            try:
                fn()
            except Exception as ex:  # noqa: BLE001 -- reported below
                errors.append(ex)
        return run

    def cells():
        for i in range(4):
            assert eng.verify_cells_batch_bytes(*c.wire(BRP, **({"cells": bad_cells} if i & 1 else {})), order=BRP) == (not i & 1)

    def openings():
        for i in range(4):
            assert eng.verify_openings_batch_bytes(*o.wire(**({"ys": bad_ys} if i & 1 else {}))) == (not i & 1)

    def blob():
        for _ in range(4):
            assert eng.verify_blobs_batch_bytes(*blob_args, order=BRP)[0]

    def commit():
        for _ in range(8):
            assert eng.commit_limbs(other).compress() == want_cm

    threads = [threading.Thread(target=guarded(f)) for f in (cells, openings, blob, cells, commit)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
