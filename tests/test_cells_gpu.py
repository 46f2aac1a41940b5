"""GPU: every cell of a domain and its multiproof (kzg_cells_and_proofs, kzg_quotient_cells) against big-integer quotients
(tests/cells_oracle.py), the existing multiproof and single-point paths bit for bit, the known secret and the pairing check."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import bigint_twin as T
import cells_oracle as CO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu
R = K.R_MODULUS
S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)


def _poly(n, seed, zeros=0):
    rnd = random.Random(seed)
    return [rnd.randrange(R) for _ in range(n)] + [0] * zeros


def _log(x):
    return x.bit_length() - 1


@pytest.fixture(scope="module")
def eng():
    e = K.Engine(0)
    yield e
    e.close()


def _check_quotients(eng, vals, K_, t, cells):
    c = K.scalars_to_limbs(vals)
    for j in cells:
        got = eng.quotient_cells_limbs(c, K_, t, j, 1)[0]
        want = CO.stride_quotient(vals, 1 << t, CO.cell_root(K_, t, j))
        assert K.limbs_to_scalars(got) == want, (K_, t, j)


@pytest.mark.parametrize("n,N,l", [(64, 128, 1), (64, 128, 8), (128, 128, 64), (100, 256, 4)])
def test_quotients_every_cell(eng, n, N, l):
    vals = _poly(n, n + N + l)
    K_, t = _log(N), _log(l)
    got = eng.quotient_cells_limbs(K.scalars_to_limbs(vals), K_, t)
    assert got.shape == (N // l, n - l, 4)
    for j in range(N // l):
        assert K.limbs_to_scalars(got[j]) == CO.stride_quotient(vals, l, CO.cell_root(K_, t, j)), j


def test_quotients_das_shape_sampled(eng):
    vals = _poly(4096, 5)
    _check_quotients(eng, vals, 13, 6, [0, 1, 63, 64, 100, 127])
    got = eng.quotient_cells_limbs(K.scalars_to_limbs(vals), 13, 6, 120, 8)  # a range at the end
    for p in range(8):
        assert K.limbs_to_scalars(got[p]) == CO.stride_quotient(vals, 64, CO.cell_root(13, 6, 120 + p))


def test_quotients_long_chain(eng):
    # l = 1, n = 2^16 + 3 (two trailing zeros): one chain of 2^16 steps in chunks of 512; the whole quotient is compared,
    # so every element on both sides of every chunk boundary is
    vals = _poly((1 << 16) + 1, 11, zeros=2)
    c = K.scalars_to_limbs(vals)
    for j in (0, 1, 77777, (1 << 17) - 1):
        got = eng.quotient_cells_limbs(c, 17, 0, j, 1)
        assert got.shape == (1, 1 << 16, 4)
        want = CO.stride_quotient(vals, 1, CO.cell_root(17, 0, j))
        assert len(want) == 1 << 16 and K.limbs_to_scalars(got[0]) == want, j


def _cell_claims(vals_limbs, K_, t, j, eng):
    zs = [K.Scalar(z) for z in CO.cell_points(K_, t, j)]
    ys = eng.evaluate_points_limbs(vals_limbs, zs)
    return zs, ys


@pytest.mark.parametrize("n,N,l", [(64, 128, 1), (64, 128, 8), (128, 128, 64), (100, 256, 4), (300, 512, 16)])
def test_proofs_equal_open_points_every_cell(engines, n, N, l):
    e = engines.bench_srs(n)
    vals = _poly(n, 3 * n + l)
    c = K.scalars_to_limbs(vals)
    K_, t = _log(N), _log(l)
    cells, proofs = e.cells_and_proofs_limbs(c, K_, t)
    assert len(proofs) == N // l
    for j in range(N // l):
        zs, ys = _cell_claims(c, K_, t, j, e)
        assert [y.v for y in ys] == K.limbs_to_scalars(cells[j * l:(j + 1) * l])
        assert np.array_equal(proofs[j].p1, e.open_points_limbs(c, zs, ys).p1), j
        if l == 1:
            assert np.array_equal(proofs[j].p1, e.open_limbs(c, zs[0], ys[0]).p1), j


@pytest.mark.parametrize("n,K_", [(4096, 13), (1 << 16, 17)])
def test_proofs_equal_open_points_sampled(engines, n, K_):
    e = engines.bench_srs(n)
    vals = _poly(n, n)
    c = K.scalars_to_limbs(vals)
    cells, proofs = e.cells_and_proofs_limbs(c, K_, 6)
    ncell = (1 << K_) >> 6
    sample = sorted(set([0, 1, ncell - 1] + random.Random(n).sample(range(ncell), 14)))
    assert len(sample) >= 16
    for j in sample:
        zs, ys = _cell_claims(c, K_, 6, j, e)
        assert [y.v for y in ys] == K.limbs_to_scalars(cells[j * 64:(j + 1) * 64])
        assert np.array_equal(proofs[j].p1, e.open_points_limbs(c, zs, ys).p1), j
    # known secret: [q_j(s)]G, one oracle multiplication each
    import oracle_ctypes as O

    for j in sample[:4]:
        q = CO.stride_quotient(vals, 64, CO.cell_root(K_, 6, j))
        assert proofs[j].compress() == TO.g1_scalar(O, CO.poly_eval(q, S)), j


def test_l1_equals_kzg_open(engines):
    n = 4096
    e = engines.bench_srs(n)
    vals = _poly(n, 21)
    c = K.scalars_to_limbs(vals)
    cells, proofs = e.cells_and_proofs_limbs(c, 12, 0)
    w = NO.domain_root(12)
    for j in (0, 1, 2, 1000, 4095):
        z = K.Scalar(pow(w, j, R))
        y = K.Scalar.from_limbs(cells[j])
        assert np.array_equal(proofs[j].p1, e.open_limbs(c, z, y).p1), j


def test_das_ordered_cell(engines):
    n = 4096
    e = engines.bench_srs(n)
    c = K.scalars_to_limbs(_poly(n, 8))
    cells, proofs = e.cells_and_proofs_limbs(c, 13, 6)
    w = NO.domain_root(13)
    for dc in (0, 5, 127):
        j, order = CO.das_cell(13, 6, dc)
        # the DAS cell's points in bit-reversed order, with its values as that order lists them
        zs = [K.Scalar(pow(w, CO.brp(dc * 64 + i, 13), R)) for i in range(64)]
        ys = [K.Scalar.from_limbs(cells[j * 64 + order[i]]) for i in range(64)]
        assert np.array_equal(e.open_points_limbs(c, zs, ys).p1, proofs[j].p1), dc


def test_known_secret_and_verification(engines, oracle):
    n = 1000
    e = engines.bench_srs(n)
    vals = _poly(n, 31)
    c = K.scalars_to_limbs(vals)
    K_, t = 11, 4
    cells, proofs = e.cells_and_proofs_limbs(c, K_, t)
    cm = e.commit_limbs(c)
    g1 = e.srs_read(0, 16)
    g2 = np.stack([K.srs_g2_at(T.BENCH_SECRET_BE, j) for j in range(17)])
    for j in (0, 3, 64, 127):
        q = CO.stride_quotient(vals, 16, CO.cell_root(K_, t, j))
        assert proofs[j].compress() == TO.g1_scalar(oracle, CO.poly_eval(q, S))
        zs = [K.Scalar(z) for z in CO.cell_points(K_, t, j)]
        ys = [K.Scalar.from_limbs(v) for v in cells[j * 16:(j + 1) * 16]]
        assert K.verify_points(cm, proofs[j], zs, ys, g1, g2)
        ys[7] = K.Scalar(ys[7].v + 1)
        assert not K.verify_points(cm, proofs[j], zs, ys, g1, g2)


def _gather(ev, K_, t):
    l = 1 << t
    return np.stack([ev[j + (i << (K_ - t))] for j in range((1 << K_) >> t) for i in range(l)])


def test_cells_equal_gathered_ntt(engines):
    e = engines.bench_srs(700)
    for n, K_, t in ((700, 10, 3), (512, 9, 0), (64, 6, 6)):
        c = K.scalars_to_limbs(_poly(n, n + K_))
        cells, _ = e.cells_and_proofs_limbs(c, K_, t)
        padded = np.zeros((1 << K_, 4), np.uint64)
        padded[:n] = c
        assert np.array_equal(cells, _gather(e.ntt_limbs(padded), K_, t))


@pytest.mark.parametrize("n,K_,t", [(256, 8, 2), (256, 9, 2), (4096, 13, 6), (64, 6, 6)])
def test_evaluations_variant(engines, n, K_, t):
    e = engines.bench_srs(n)
    ev = K.scalars_to_limbs(_poly(n, n * 3 + K_))
    coeffs = e.intt_limbs(ev)
    cells_a, proofs_a = e.cells_and_proofs_from_evaluations_limbs(ev, K_, t)
    cells_b, proofs_b = e.cells_and_proofs_limbs(coeffs, K_, t)
    assert np.array_equal(cells_a, cells_b)
    assert all(np.array_equal(a.p1, b.p1) for a, b in zip(proofs_a, proofs_b))
    if K_ == _log(n):  # N = n: the cells are the values themselves, gathered
        assert np.array_equal(cells_a, _gather(ev, K_, t))


def _inf(p):
    return not p.p1.any()


def test_short_and_empty_inputs(engines):
    e = engines.bench_srs(100)
    for n in (0, 1, 8):  # n' <= l = 8: infinity proofs
        vals = _poly(n, n)
        cells, proofs = e.cells_and_proofs_limbs(K.scalars_to_limbs(vals) if n else np.zeros((0, 4), np.uint64), 6, 3)
        assert len(proofs) == 8 and all(_inf(p) for p in proofs)
        assert K.limbs_to_scalars(cells) == CO.cells(vals, 6, 3)
    # a constant with trailing zeros far past srs_len + l, and a polynomial whose zeros start right after srs_len + l
    c = K.scalars_to_limbs([5] + [0] * 1000)
    cells, proofs = e.cells_and_proofs_limbs(c, 11, 2)
    assert all(_inf(p) for p in proofs) and K.limbs_to_scalars(cells) == [5] * 2048
    vals = _poly(104, 4) + [0] * 900
    _, proofs = e.cells_and_proofs_limbs(K.scalars_to_limbs(vals), 10, 2)
    q = CO.stride_quotient(vals, 4, CO.cell_root(10, 2, 9))
    assert len(q) == 100 and proofs[9].compress() == TO.g1_scalar(__import__("oracle_ctypes"), CO.poly_eval(q, S))


def test_degree_and_argument_errors(engines, eng):
    srs_len = 100
    e = engines.bench_srs(srs_len)
    l = 4
    e.cells_and_proofs_limbs(K.scalars_to_limbs(_poly(srs_len + l, 1)), 8, 2)  # n' - l = srs_len
    with pytest.raises(K.KzgError) as ei:
        e.cells_and_proofs_limbs(K.scalars_to_limbs(_poly(srs_len + l + 1, 1)), 8, 2)
    assert ei.value.status == K.KZG_ERR_DEGREE_TOO_HIGH
    c = K.scalars_to_limbs(_poly(64, 2))
    for K_, t, n in ((23, 0, 64), (10, 7, 64), (3, 4, 8), (5, 0, 64)):  # log N, log l > 6, l > N, n > N
        with pytest.raises(K.KzgError) as ei:
            e.cells_and_proofs_limbs(c[:n], K_, t)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG, (K_, t, n)
        with pytest.raises(K.KzgError) as ei:
            e.quotient_cells_limbs(c[:n], K_, t, 0, 0)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG, (K_, t, n)
    for n in (3, 48):  # not a power of two
        with pytest.raises(K.KzgError) as ei:
            e.cells_and_proofs_from_evaluations_limbs(c[:n], 7, 2)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
    lib = K.load_library()
    out = np.zeros((64, 18), np.uint64)
    ptr = c.ctypes.data_as(C.c_void_p)
    assert lib.kzg_cells_and_proofs(e._h, ptr, 64, 8, 2, None, None) == K.KZG_ERR_INVALID_ARG  # out_proofs
    assert lib.kzg_cells_and_proofs(e._h, None, 64, 8, 2, None, out.ctypes.data_as(C.c_void_p)) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_cells_and_proofs(None, ptr, 64, 8, 2, None, out.ctypes.data_as(C.c_void_p)) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_cells_and_proofs_evaluations(e._h, None, 64, 8, 2, None, out.ctypes.data_as(C.c_void_p)) == K.KZG_ERR_INVALID_ARG
    qn = C.c_size_t(0)
    assert lib.kzg_quotient_cells(e._h, ptr, 64, 8, 2, 60, 5, None, C.byref(qn)) == K.KZG_ERR_INVALID_ARG  # past the cells
    assert lib.kzg_quotient_cells(e._h, ptr, 64, 8, 2, 0, 1, None, C.byref(qn)) == K.KZG_ERR_INVALID_ARG  # out_q
    assert lib.kzg_quotient_cells(e._h, ptr, 64, 8, 2, 0, 1, out.ctypes.data_as(C.c_void_p), None) == K.KZG_ERR_INVALID_ARG
    # no SRS (argument errors come first)
    for fn in (eng.cells_and_proofs_limbs, eng.cells_and_proofs_from_evaluations_limbs):
        with pytest.raises(K.KzgError) as ei:
            fn(c, 8, 2)
        assert ei.value.status == K.KZG_ERR_NO_SRS
    assert eng.quotient_cells_limbs(c, 8, 2, 0, 2).shape == (2, 60, 4)  # the test hook needs no SRS


def test_sub_batches_and_concurrency(oracle):
    n = 512
    vals = _poly(n, 99)
    c = K.scalars_to_limbs(vals)
    results = {}
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(n)
    try:
        for b in (1, 7, 128):  # 7: a ragged last sub-batch of the 64 cells
            e.set_max_batch(b)
            cells, proofs = e.cells_and_proofs_limbs(c, 10, 4)
            results[b] = (cells, np.stack([p.p1 for p in proofs]))
        for b in (7, 128):
            assert np.array_equal(results[b][0], results[1][0]) and np.array_equal(results[b][1], results[1][1]), b
        # two threads proving cells while a third commits on the same context
        e.set_max_batch(7)
        other = K.scalars_to_limbs(_poly(300, 5))
        want_cm = e.commit_limbs(other).compress()
        errors, stop = [], threading.Event()

        def prove(seed):
            try:
                mine = K.scalars_to_limbs(_poly(n, seed))
                ref_cells, ref_proofs = e.cells_and_proofs_limbs(mine, 10, 4)
                for _ in range(3):
                    cells, proofs = e.cells_and_proofs_limbs(mine, 10, 4)
                    assert np.array_equal(cells, ref_cells)
                    assert all(np.array_equal(a.p1, b.p1) for a, b in zip(proofs, ref_proofs))
                j = 17
                q = CO.stride_quotient(K.limbs_to_scalars(mine), 16, CO.cell_root(10, 4, j))
                assert ref_proofs[j].compress() == TO.g1_scalar(oracle, CO.poly_eval(q, S))
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
        ts = [threading.Thread(target=prove, args=(s,)) for s in (1, 2)]
        for th in ts:
            th.start()
        for th in ts:
            th.join()
        stop.set()
        cl.join()
        assert not errors, errors
    finally:
        e.close()


def test_multi_device_contexts():
    n = 1000
    c = K.scalars_to_limbs(_poly(n, 123))
    single = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(n)
    try:
        want_cells, want = single.cells_and_proofs_limbs(c, 11, 5)
    finally:
        single.close()
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(T.BENCH_SECRET_BE, n)
        cells, got = rep.cells_and_proofs_limbs(c, 11, 5)
        assert np.array_equal(cells, want_cells)
        assert all(np.array_equal(a.p1, b.p1) for a, b in zip(got, want))
    finally:
        rep.close()
    rng = K.Engine(devices=[0, 0])
    try:
        rng.srs_generate(T.BENCH_SECRET_BE, n)
        with pytest.raises(K.KzgError) as ei:
            rng.cells_and_proofs_limbs(c, 11, 5)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        assert b"range-split" in K.load_library().kzg_last_error(rng._h)
        assert rng.quotient_cells_limbs(c, 11, 5, 3, 2).shape == (2, n - 32, 4)
    finally:
        rng.close()
