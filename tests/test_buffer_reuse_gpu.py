"""GPU: one engine driven through every family of device and pinned buffers in the order small, large, small, so that each
buffer is created, grown, and then reused while larger than the call needs ("Who owns which memory"),
with the SRS replaced in the middle.  Every result is checked the way its family's own test checks it -- the host verifiers,
or scalars of the trapdoor oracle -- and must be byte-equal to the same call on a fresh engine.  At the end the engine is
closed and a second one is created, used and closed in the same process."""
import random

import numpy as np
import pytest

import bigint_twin as T
import blob_oracle as BO
import cells_oracle as CO
import kzg_poly_commit_exploration_amd as K
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu
R = K.R_MODULUS
S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)
G2 = np.stack([K.srs_g2_at(T.BENCH_SECRET_BE, j) for j in range(17)])


def _poly(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R) for _ in range(n)]


def _points(k, seed):
    return [K.Scalar(v) for v in _poly(k, 9000 + seed)]  # (distinct: k random values below r)


def _values(vals, zs):
    return [K.Scalar(TO.poly_eval(vals, z.v)) for z in zs]


def _raw(points):
    return b"".join(p.p1.tobytes() for p in points)


def _commitments_hold(oracle, commitments, polys):
    return all(c.compress() == TO.commitment(oracle, p, S) for c, p in zip(commitments, polys))


# ---- one call of each family: runs it on e, checks the result when asked to, returns the result's bytes ----------------------
def open_points(k):
    def run(e, oracle, check):
        vals = _poly(40, 100 + k)
        c, zs = K.scalars_to_limbs(vals), _points(k, k)
        ys = _values(vals, zs)
        cm, pi = e.commit_limbs(c), e.open_points_limbs(c, zs, ys)
        if check:
            assert _commitments_hold(oracle, [cm], [vals])
            assert K.verify_points(cm, pi, zs, ys, e.srs_read(0, 16), G2)
        return _raw([cm, pi])
    return run


def open_combined(t, n):
    def run(e, oracle, check):
        polys = [_poly(n, 200 + 1000 * n + i) for i in range(t)]
        a = np.stack([K.scalars_to_limbs(p) for p in polys])
        z, gamma = _points(2, 31 * t + n)
        ys, pi = e.open_combined_limbs(a, z, gamma)
        cms = e.commit_batch_host(a)
        if check:
            assert [y.v for y in ys] == [TO.poly_eval(p, z.v) for p in polys]
            assert _commitments_hold(oracle, cms, polys)
            assert K.verify_combined(cms, ys, z, gamma, pi, G2[1])
        return _raw(cms + [pi]) + b"".join(y.limbs().tobytes() for y in ys)
    return run


def open_sets(nsets):
    def run(e, oracle, check):
        pts = _points(2 * nsets, 70 + nsets)
        # one set of one point, or sets of three points that share one with the next set: 2 * nsets distinct points
        sets = [[pts[0]]] if nsets == 1 else [[pts[2 * g], pts[2 * g + 1], pts[(2 * g + 2) % len(pts)]] for g in range(nsets)]
        set_of = list(range(nsets))
        polys = [_poly(40, 300 + 10 * nsets + i) for i in range(nsets)]
        a = np.stack([K.scalars_to_limbs(p) for p in polys])
        gamma = _points(1, 80 + nsets)[0]
        ys, pi = e.open_sets_limbs(a, set_of, sets, gamma)
        cms = e.commit_batch_host(a)
        if check:
            assert [[y.v for y in row] for row in ys] == [[TO.poly_eval(p, z.v) for z in sets[g]] for p, g in zip(polys, set_of)]
            assert _commitments_hold(oracle, cms, polys)
            assert K.verify_sets(cms, set_of, sets, ys, gamma, pi, e.srs_read(0, 16), G2)
        return _raw(cms + [pi])
    return run


def open_batch(b):
    def run(e, oracle, check):
        if e.max_batch() < b:
            assert e.set_max_batch(b) == b
        polys = [_poly(60, 400 + 10 * b + i) for i in range(b)]
        limbs = [K.scalars_to_limbs(p) for p in polys]
        zs = _points(b, 90 + b)
        ys = [_values(p, [z])[0] for p, z in zip(polys, zs)]
        proofs = e.open_batch_limbs(limbs, zs, ys)
        cms = e.commit_batch_limbs(limbs)
        assert all(isinstance(p, K.G1Point) for p in proofs), proofs
        if check:
            assert _commitments_hold(oracle, cms, polys)
            assert K.verify_proof_batch(cms, proofs, zs, ys, G2[1]) == [True] * b
        return _raw(cms + proofs)
    return run


def _cell_proofs_hold(oracle, proofs, vals, K_, t):
    q = TO.cell_proof_scalars_fast(CO.trim(vals) or [0], K_, t, S)
    return all(p.compress() == TO.g1_scalar(oracle, q[j]) for j, p in enumerate(proofs))


def fk20(t):
    K_, n = 7, 64

    def run(e, oracle, check):
        polys = [_poly(n, 500 + b) for b in range(2)]
        c = np.stack([K.scalars_to_limbs(p) for p in polys])
        cells, proofs = e.cells_and_proofs_fk20(c, K_, t)
        if check:
            l = 1 << t
            for b in range(2):
                assert K.limbs_to_scalars(cells[b]) == CO.cells(polys[b], K_, t), b
                assert _cell_proofs_hold(oracle, proofs[b], polys[b], K_, t), b
            cm, j = e.commit_limbs(c[1]), 5
            zs = [K.Scalar(z) for z in CO.cell_points(K_, t, j)]
            ys = [K.Scalar.from_limbs(v) for v in cells[1][j * l:(j + 1) * l]]
            assert K.verify_points(cm, proofs[1][j], zs, ys, e.srs_read(0, 16), G2)
        return cells.tobytes() + _raw(proofs[0] + proofs[1])
    return run


def recover(K_):
    t = 2

    def run(e, oracle, check):
        N, l = 1 << K_, 1 << t
        n, M = N // 2, N >> t
        polys = [_poly(n, 600 + K_ + b) for b in range(2)]
        cells = [CO.cells(p, K_, t) for p in polys]
        ids = random.Random(K_).sample(range(M), M // 2)
        rx = np.stack([np.stack([K.scalars_to_limbs(cl[j * l:(j + 1) * l]) for j in ids]) for cl in cells])
        co, ce, pr = e.recover_cells_and_proofs(n, K_, t, ids, rx)
        if check:
            for b in range(2):
                assert K.limbs_to_scalars(co[b]) == polys[b], b
                assert K.limbs_to_scalars(ce[b]) == cells[b], b
                assert _cell_proofs_hold(oracle, pr[b], polys[b], K_, t), b
        return co.tobytes() + ce.tobytes() + _raw(pr[0] + pr[1])
    return run


_RECORDS = {}


def _cell_records(oracle):
    """32 valid records (2 polynomials x 16 cells of 8 values) made without the library's device side"""
    if not _RECORDS:
        K_, t, l = 7, 3, 8
        polys = [_poly(64, 700 + b) for b in range(2)]
        _RECORDS["coms"] = [K.G1Point.uncompress(TO.commitment(oracle, p, S)) for p in polys]
        rows = []
        for b, p in enumerate(polys):
            cells = CO.cells(p, K_, t)
            q = TO.cell_proof_scalars_fast(p, K_, t, S)
            for j in range(16):
                rows.append((b, j, K.scalars_to_limbs(cells[j * l:(j + 1) * l]), K.G1Point.uncompress(TO.g1_scalar(oracle, q[j]))))
        random.Random(7).shuffle(rows)
        _RECORDS["rows"] = rows
    return _RECORDS["coms"], _RECORDS["rows"]


def verify_cells(k):
    def run(e, oracle, check):
        coms, rows = _cell_records(oracle)
        idx, ids, vals, prf = zip(*rows[:k])
        ok = e.verify_cells_batch(coms, idx, ids, np.stack(vals), prf, 7, 3, G2[:9])
        wrong = np.stack(vals).copy()
        wrong[k - 1, 3, 0] ^= 1  # another (still canonical) value in the last record
        bad = e.verify_cells_batch(coms, idx, ids, wrong, prf, 7, 3, G2[:9])
        if check:
            assert ok and not bad
        return bytes([ok, bad])
    return run


def blobs(batch):
    n, K_, t = 16, 5, 2

    def run(e, oracle, check):
        rnd = random.Random(800 + batch)
        data = [b"".join(rnd.randrange(R).to_bytes(32, "big") for _ in range(n)) for _ in range(batch)]
        coms, cells, proofs = e.blobs_to_cells_and_proofs_bytes(b"".join(data), n, K_, t)
        if check:
            want = [b"", b"", b""]
            for blob in data:
                c = BO.blob_coefficients(blob, K.KZG_ORDER_NATURAL)
                q = TO.cell_proof_scalars_fast(CO.trim(c) or [0], K_, t, S)
                want[0] += TO.commitment(oracle, c, S)
                want[1] += BO.cells_bytes(c, K_, t, K.KZG_ORDER_NATURAL)
                want[2] += b"".join(TO.g1_scalar(oracle, q[j]) for j in range((1 << K_) >> t))
            assert [coms, cells, proofs] == want
        return coms + cells + proofs
    return run


# every family small, large, small (the combined openings once with 16 and once with 200 coefficients)
FAMILIES = [
    [("points 2", open_points(2)), ("points 16", open_points(16))],
    [("combined 2x16", open_combined(2, 16)), ("combined 40x16", open_combined(40, 16))],
    [("combined 2x200", open_combined(2, 200)), ("combined 40x200", open_combined(40, 200))],
    [("sets 1", open_sets(1)), ("sets 8", open_sets(8))],
    [("batch 1", open_batch(1)), ("batch 4", open_batch(4))],
    [("fk20 cells of 2", fk20(1)), ("fk20 cells of 8", fk20(3))],
    [("recover 16", recover(4)), ("recover 64", recover(6))],
    [("verify 2", verify_cells(2)), ("verify 24", verify_cells(24))],
    [("blobs 1", blobs(1)), ("blobs 3", blobs(3))],
]
# the first small calls, repeated after each SRS replacement (the combined opening of 200 coefficients needs the longer SRS)
SMALL = [small for small, _ in FAMILIES if small[0] != "combined 2x200"]


def test_buffers_are_created_grown_and_reused(oracle):
    fresh = {}

    def reference(name, run, srs_len):
        """the bytes of the same call on an engine that has done nothing else (made once per call and SRS length)"""
        if (name, srs_len) not in fresh:
            f = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(srs_len)
            try:
                fresh[name, srs_len] = run(f, oracle, False)
            finally:
                f.close()
        return fresh[name, srs_len]

    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(256)
    try:
        def step(call, srs_len=256):
            name, run = call
            assert e.srs_len() == srs_len
            assert run(e, oracle, True) == reference(name, run, srs_len), name

        for small, large in FAMILIES:
            step(small)
            step(large)
            step(small)
        for srs_len in (128, 256):  # the grown buffers survive an SRS replacement; the MSM workspaces are made again
            e.srs_generate(T.BENCH_SECRET_BE, srs_len)
            for call in SMALL:
                step(call, srs_len)
    finally:
        e.close()
    # destruction leaves the device usable: a second engine in the same process, one commitment, closed again
    second = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(256)
    try:
        vals = _poly(256, 1)
        assert second.commit_limbs(K.scalars_to_limbs(vals)).compress() == TO.commitment(oracle, vals, S)
    finally:
        second.close()
