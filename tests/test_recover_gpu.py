"""GPU: kzg_recover_cells_and_proofs.  Recovered coefficients against the originals and tests/recover_oracle.py, recovered cells
and proofs against kzg_cells_and_proofs_fk20 of the originals byte for byte, the known secret and the pairing check; the
bit-reversed sampling order, pass and shape boundaries, every error, multi-device contexts and a concurrent commitment."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import bigint_twin as T
import cells_oracle as CO
import kzg_poly_commit_exploration_amd as K
import recover_oracle as RO
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu
R = K.R_MODULUS
S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)


def _poly(n, seed, zeros=0):
    rnd = random.Random(seed)
    return [rnd.randrange(R) for _ in range(n)] + [0] * zeros


def _stack(points):
    return np.stack([p.p1 for p in points]) if points else np.zeros((0, 18), np.uint64)


def _received(all_cells, ids, t):
    """(batch, N, 4) cell-major values -> (batch, k, l, 4) of the cells ids, in that order"""
    a = np.asarray(all_cells)
    b, N = a.shape[0], a.shape[1]
    return np.ascontiguousarray(a.reshape(b, N >> t, 1 << t, 4)[:, list(ids)])


def _min_cells(n, l):
    return -(-n // l)


@pytest.fixture(scope="module")
def das():
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(4096)
    yield e
    e.close()


@pytest.fixture(scope="module")
def nosrs():
    e = K.Engine(0)
    yield e
    e.close()


# ---- the DAS shape: (n, N, l) = (4096, 8192, 64), half of the cells ---------------------------------------------------------
def test_das_shape_against_fk20(das, oracle):
    n, K_, t, batch = 4096, 13, 6, 4
    polys = [_poly(n, 100 + b) for b in range(batch)]
    c = np.stack([K.scalars_to_limbs(p) for p in polys])
    want_cells, want_proofs = das.cells_and_proofs_fk20(c, K_, t)
    ids = random.Random(1).sample(range(128), 64)  # shuffled
    co, ce, pr = das.recover_cells_and_proofs(n, K_, t, ids, _received(want_cells, ids, t))
    assert np.array_equal(co, c)
    assert np.array_equal(ce, want_cells)
    for b in range(batch):
        assert np.array_equal(_stack(pr[b]), _stack(want_proofs[b])), b
    for j in (0, 77, 127):
        q = CO.stride_quotient(polys[0], 64, CO.cell_root(K_, t, j))
        assert pr[0][j].compress() == TO.g1_scalar(oracle, CO.poly_eval(q, S)), j
    cm = das.commit_limbs(c[1])
    g1 = das.srs_read(0, 64)
    g2 = np.stack([K.srs_g2_at(T.BENCH_SECRET_BE, j) for j in range(65)])
    j = ids[-1] ^ 1
    zs = [K.Scalar(z) for z in CO.cell_points(K_, t, j)]
    ys = [K.Scalar.from_limbs(v) for v in ce[1][j * 64:(j + 1) * 64]]
    assert K.verify_points(cm, pr[1][j], zs, ys, g1, g2)


def test_trailing_zeros_and_short_polynomials(das):
    """n' < n, n' <= l (infinity proofs) and n' = 0 at the DAS shape, against FK20 of the originals"""
    n, K_, t = 4096, 13, 6
    polys = [_poly(keep, 200 + keep) + [0] * (n - keep) for keep in (4096, 1000, 64, 5, 0)]
    c = np.stack([K.scalars_to_limbs(p) for p in polys])
    want_cells, want_proofs = das.cells_and_proofs_fk20(c, K_, t)
    ids = random.Random(2).sample(range(128), 64)
    co, ce, pr = das.recover_cells_and_proofs(n, K_, t, ids, _received(want_cells, ids, t))
    assert np.array_equal(co, c) and np.array_equal(ce, want_cells)
    for b in range(len(polys)):
        assert np.array_equal(_stack(pr[b]), _stack(want_proofs[b])), b
    assert all(p.is_infinity() for p in pr[2] + pr[3] + pr[4])


# ---- small shapes against the oracle --------------------------------------------------------------------------------------
def _sweep():
    for K_ in range(0, 7):
        for t in range(0, K_ + 1):
            N, l = 1 << K_, 1 << t
            for n in sorted({1, l, N // 2, N - l, N}):
                if 1 <= n <= N:
                    yield K_, t, n


@pytest.mark.parametrize("K_,t", sorted({(k, t) for k, t, _ in _sweep()}))
def test_small_shapes_against_oracle(engines, K_, t):
    e = engines.bench_srs(64)
    N, l = 1 << K_, 1 << t
    M = N >> t
    for n in sorted({n for k, tt, n in _sweep() if (k, tt) == (K_, t)}):
        rnd = random.Random(K_ * 1000 + t * 100 + n)
        polys = [_poly(n, 300 + b + n) for b in range(2)]
        k = min(M, _min_cells(n, l) + rnd.randrange(2))
        ids = rnd.sample(range(M), k)
        cells = [CO.cells(p, K_, t) for p in polys]
        rx = np.stack([np.stack([K.scalars_to_limbs(cl[j * l:(j + 1) * l]) for j in ids]) for cl in cells])
        want = [RO.decode(n, K_, t, ids, [cl[j * l:(j + 1) * l] for j in ids]) for cl in cells]
        co, ce, pr = e.recover_cells_and_proofs(n, K_, t, ids, rx, proofs=(n == max(1, N - l)))
        for b in range(2):
            assert want[b] == (polys[b], True)
            assert K.limbs_to_scalars(co[b]) == polys[b], (n, b)
            assert K.limbs_to_scalars(ce[b]) == cells[b], (n, b)
        if pr is not None:
            _, fk = e.cells_and_proofs_fk20(np.stack([K.scalars_to_limbs(p) for p in polys]), K_, t, cells=False)
            for b in range(2):
                assert np.array_equal(_stack(pr[b]), _stack(fk[b])), (n, b)


def test_bit_reversed_sampling_round_trip(engines):
    """a sampling spec lists the N values in bit-reversed order: its cell c is our cell brp_(K-t)(c), values in brp_t order"""
    e = engines.bench_srs(64)
    K_, t, n = 6, 2, 32
    N, l = 1 << K_, 1 << t
    M = N >> t
    poly = _poly(n, 5)
    ev = CO.cells(poly, K_, t)  # ours, to build the spec list from the points themselves
    w = [None] * N
    for j in range(M):
        for i in range(l):
            w[j + M * i] = ev[j * l + i]
    spec = [w[CO.brp(p, K_)] for p in range(N)]  # spec position p holds P(w_N^brp_K(p))
    spec_cells = random.Random(6).sample(range(M), 9)
    ids, rows = [], []
    for c in spec_cells:
        j, order = CO.das_cell(K_, t, c)
        assert j == CO.brp(c, K_ - t)
        ids.append(j)
        vals = spec[c * l:(c + 1) * l]
        ours = [0] * l
        for i in range(l):
            ours[order[i]] = vals[i]
        rows.append(K.scalars_to_limbs(ours))
    co, ce, _ = e.recover_cells_and_proofs(n, K_, t, ids, np.stack(rows), proofs=False)
    assert K.limbs_to_scalars(co[0]) == poly
    got = K.limbs_to_scalars(ce[0])
    for c in range(M):
        j, order = CO.das_cell(K_, t, c)
        assert [got[j * l + order[i]] for i in range(l)] == spec[c * l:(c + 1) * l], c


# ---- boundaries ---------------------------------------------------------------------------------------------------------
def test_largest_cell_count(das):
    """M = 2^13 cells of one point (N = 8192), half of them missing"""
    n, K_, t = 4096, 13, 0
    polys = [_poly(n, 400 + b) for b in range(2)]
    c = np.stack([K.scalars_to_limbs(p) for p in polys])
    want_cells, want_proofs = das.cells_and_proofs_fk20(c, K_, t)
    ids = random.Random(3).sample(range(8192), 4096)
    co, ce, pr = das.recover_cells_and_proofs(n, K_, t, ids, _received(want_cells, ids, t))
    assert np.array_equal(co, c) and np.array_equal(ce, want_cells)
    for b in range(2):
        assert np.array_equal(_stack(pr[b]), _stack(want_proofs[b])), b


def test_batch_crosses_passes(engines):
    """130 polynomials: three passes of at most 64"""
    e = engines.bench_srs(64)
    K_, t, n, batch = 4, 1, 8, 130
    polys = [_poly(n, 500 + b) for b in range(batch)]
    c = np.stack([K.scalars_to_limbs(p) for p in polys])
    want_cells, want_proofs = e.cells_and_proofs_fk20(c, K_, t)
    ids = [7, 2, 5, 0, 6]
    co, ce, pr = e.recover_cells_and_proofs(n, K_, t, ids, _received(want_cells, ids, t))
    assert np.array_equal(co, c) and np.array_equal(ce, want_cells)
    for b in range(batch):
        assert np.array_equal(_stack(pr[b]), _stack(want_proofs[b])), b


def test_empty_batch_and_selective_outputs(engines):
    e = engines.bench_srs(64)
    lib = K.load_library()
    K_, t, n = 5, 2, 16
    polys = [_poly(n, 600 + b) for b in range(3)]
    c = np.stack([K.scalars_to_limbs(p) for p in polys])
    want_cells, want_proofs = e.cells_and_proofs_fk20(c, K_, t)
    ids = np.array([3, 1, 6, 4, 0], dtype=np.uint32)
    rx = _received(want_cells, ids, t)
    ip, xp = ids.ctypes.data_as(C.c_void_p), rx.ctypes.data_as(C.c_void_p)
    assert lib.kzg_recover_cells_and_proofs(e._h, n, K_, t, ip, 5, xp, 0, None, None, None) == K.KZG_OK
    assert lib.kzg_recover_cells_and_proofs(e._h, n, K_, t, ip, 5, None, 0, None, None, None) == K.KZG_OK
    assert lib.kzg_recover_cells_and_proofs(e._h, n, K_, t, ip, 5, xp, 3, None, None, None) == K.KZG_OK  # validates only
    for want_c in (False, True):
        for want_v in (False, True):
            for want_p in (False, True):
                co, ce, pr = e.recover_cells_and_proofs(n, K_, t, ids, rx, coeffs=want_c, cells_out=want_v, proofs=want_p)
                assert (co is not None) == want_c and (ce is not None) == want_v and (pr is not None) == want_p
                if want_c:
                    assert np.array_equal(co, c)
                if want_v:
                    assert np.array_equal(ce, want_cells)
                if want_p:
                    for b in range(3):
                        assert np.array_equal(_stack(pr[b]), _stack(want_proofs[b]))


# ---- errors -------------------------------------------------------------------------------------------------------------
def test_corrupted_polynomial_is_named(engines):
    e = engines.bench_srs(64)
    lib = K.load_library()
    K_, t, n = 6, 2, 32
    polys = [_poly(n, 700 + b) for b in range(4)]
    c = np.stack([K.scalars_to_limbs(p) for p in polys])
    want_cells, _ = e.cells_and_proofs_fk20(c, K_, t, cells=True)
    ids = random.Random(7).sample(range(16), 10)
    rx = _received(want_cells, ids, t)
    rx[2, 4, 1] = K.scalars_to_limbs([K.limbs_to_scalars(rx[2, 4, 1])[0] + 1])[0]
    for flags in ((True, True, True), (True, False, False), (False, False, False)):
        with pytest.raises(K.KzgError) as ei:
            e.recover_cells_and_proofs(n, K_, t, ids, rx, *flags)
        assert ei.value.status == K.KZG_ERR_REMAINDER
        assert b"polynomial 2" in lib.kzg_last_error(e._h)


def test_invalid_arguments(engines):
    e = engines.bench_srs(64)
    lib = K.load_library()
    good = np.zeros((2, 8, 4, 4), np.uint64)
    ids = np.arange(8, dtype=np.uint32)
    ip, xp = ids.ctypes.data_as(C.c_void_p), good.ctypes.data_as(C.c_void_p)
    out = np.zeros((2, 1 << 20, 4), np.uint64)
    op = out.ctypes.data_as(C.c_void_p)

    def call(n, K_, t, ids_p=ip, k=8, cells_p=xp, batch=2):
        return lib.kzg_recover_cells_and_proofs(e._h, n, K_, t, ids_p, k, cells_p, batch, op, None, None)

    assert call(32, 6, 2) == K.KZG_OK
    for args in ((32, 23, 2), (32, 6, 7), (2, 1, 2), (32, 20, 6), (0, 6, 2), (65, 6, 2), (33, 6, 2)):
        assert call(*args) == K.KZG_ERR_INVALID_ARG, args  # log N, log l, l > N, M > 2^13, n = 0, n > N, k l < n
    far = np.array([0, 1, 2, 3, 4, 5, 6, 16], dtype=np.uint32)  # 16 >= M = 16
    assert call(32, 6, 2, ids_p=far.ctypes.data_as(C.c_void_p)) == K.KZG_ERR_INVALID_ARG
    dup = np.array([0, 1, 2, 3, 4, 5, 6, 6], dtype=np.uint32)
    assert call(32, 6, 2, ids_p=dup.ctypes.data_as(C.c_void_p)) == K.KZG_ERR_INVALID_ARG
    assert b"twice" in lib.kzg_last_error(e._h)
    assert call(32, 6, 2, ids_p=None) == K.KZG_ERR_INVALID_ARG
    assert call(32, 6, 2, cells_p=None) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_recover_cells_and_proofs(None, 32, 6, 2, ip, 8, xp, 2, op, None, None) == K.KZG_ERR_INVALID_ARG
    big = good.copy()
    big[1, 5, 3] = [0xFFFFFFFF00000001, 0x53BDA402FFFE5BFE, 0x3339D80809A1D805, 0x73EDA753299D7D48]  # r itself
    assert call(32, 6, 2, cells_p=big.ctypes.data_as(C.c_void_p)) == K.KZG_ERR_INVALID_ARG
    msg = lib.kzg_last_error(e._h)
    assert b"polynomial 1" in msg and b"cell 5" in msg


def test_srs_errors(oracle, nosrs):
    K_, t, n = 7, 2, 128
    poly = _poly(n, 800)
    cells = CO.cells(poly, K_, t)
    ids = list(range(0, 32, 1))
    rx = np.stack([K.scalars_to_limbs(cells[j * 4:(j + 1) * 4]) for j in ids])
    short = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(50)  # n' - l = 124 > 50
    try:
        with pytest.raises(K.KzgError) as ei:
            short.recover_cells_and_proofs(n, K_, t, ids, rx)
        assert ei.value.status == K.KZG_ERR_DEGREE_TOO_HIGH
        co, ce, _ = short.recover_cells_and_proofs(n, K_, t, ids, rx, proofs=False)
        assert K.limbs_to_scalars(co[0]) == poly and K.limbs_to_scalars(ce[0]) == cells
    finally:
        short.close()
    with pytest.raises(K.KzgError) as ei:
        nosrs.recover_cells_and_proofs(n, K_, t, ids, rx)
    assert ei.value.status == K.KZG_ERR_NO_SRS
    co, ce, pr = nosrs.recover_cells_and_proofs(n, K_, t, ids, rx, proofs=False)
    assert K.limbs_to_scalars(co[0]) == poly and K.limbs_to_scalars(ce[0]) == cells and pr is None


# ---- multi-device, concurrency --------------------------------------------------------------------------------------------
def test_multi_device_contexts():
    n, K_, t = 1000, 11, 5
    poly = _poly(n, 900)
    c = K.scalars_to_limbs(poly)
    single = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(n)
    try:
        want_cells, want = single.cells_and_proofs_fk20(c, K_, t)
    finally:
        single.close()
    ids = random.Random(9).sample(range(64), 40)
    rx = _received(want_cells, ids, t)
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(T.BENCH_SECRET_BE, n)
        co, ce, pr = rep.recover_cells_and_proofs(n, K_, t, ids, rx)
        assert np.array_equal(co[0], c) and np.array_equal(ce, want_cells)
        assert np.array_equal(_stack(pr[0]), _stack(want[0]))
    finally:
        rep.close()
    rng = K.Engine(devices=[0, 0])
    try:
        rng.srs_generate(T.BENCH_SECRET_BE, n)
        with pytest.raises(K.KzgError) as ei:
            rng.recover_cells_and_proofs(n, K_, t, ids, rx)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        assert b"range-split" in K.load_library().kzg_last_error(rng._h)
    finally:
        rng.close()


def test_recovery_beside_commitments():
    n, K_, t = 512, 10, 3
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(n)
    try:
        other = K.scalars_to_limbs(_poly(300, 5))
        want_cm = e.commit_limbs(other).compress()
        c = np.stack([K.scalars_to_limbs(_poly(n, 950 + b)) for b in range(3)])
        want_cells, want_proofs = e.cells_and_proofs_fk20(c, K_, t)
        ids = random.Random(10).sample(range(128), 70)
        rx = _received(want_cells, ids, t)
        errors, stop = [], threading.Event()

        def recover():
            try:
                for _ in range(3):
                    co, ce, pr = e.recover_cells_and_proofs(n, K_, t, ids, rx)
                    assert np.array_equal(co, c) and np.array_equal(ce, want_cells)
                    for b in range(3):
                        assert np.array_equal(_stack(pr[b]), _stack(want_proofs[b]))
            except Exception as ex:  # noqa: BLE001 -- reported below
                errors.append(ex)

        def commit_loop():
            try:
                while not stop.is_set():
                    assert e.commit_limbs(other).compress() == want_cm
            except Exception as ex:  # noqa: BLE001
                errors.append(ex)

        cl = threading.Thread(target=commit_loop)
        cl.start()
        rt = threading.Thread(target=recover)
        rt.start()
        rt.join()
        stop.set()
        cl.join()
        assert not errors, errors
    finally:
        e.close()
