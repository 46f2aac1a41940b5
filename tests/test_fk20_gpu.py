"""GPU: FK20 (kzg_cells_and_proofs_fk20, kzg_fk20_prepare) and the G1 DFT under it (kzg_g1_dft): the DFT against
big-integer group arithmetic and against the known scalars of SRS points, and every FK20 output against
kzg_cells_and_proofs byte for byte, the known secret and the pairing check."""
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


def _stack(points):
    return np.stack([p.p1 for p in points]) if points else np.zeros((0, 18), np.uint64)


@pytest.fixture(scope="module")
def eng():
    e = K.Engine(0)
    yield e
    e.close()


# ---- the G1 DFT ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 4, 8, 16])
def test_g1_dft_against_group_law(eng, m):
    rnd = random.Random(m)
    g = T.srs_g1(T.BENCH_SECRET_BE, 2)[1]
    pts = [T.g1_mul(g, rnd.randrange(1, R)) for _ in range(m)]
    if m >= 4:
        pts[2] = T.INF
        pts[3] = pts[1]  # equal inputs: the butterflies meet P + P and P - P
    inp = np.stack([np.array(T.g1_to_blst_p1_limbs(p), dtype=np.uint64) if p is not T.INF else np.zeros(18, np.uint64)
                    for p in pts])
    w = NO.domain_root(_log(m))
    got = eng.g1_dft(inp)
    for j in range(m):
        want = T.INF
        for i, p in enumerate(pts):
            want = T.g1_add(want, T.g1_mul(p, pow(w, i * j, R)) if p is not T.INF else T.INF)
        assert got[j].compress() == T.g1_compress(want), (m, j)
    back = eng.g1_dft(got, inverse=True)
    assert [p.compress() for p in back] == [T.g1_compress(p) for p in pts]


@pytest.mark.parametrize("m", [32, 1 << 10, 1 << 13])
def test_g1_dft_known_scalars(engines, oracle, m):
    e = engines.bench_srs(m)
    inp = e.srs_read(0, m)  # [s^i]G
    xs = [pow(S, i, R) for i in range(m)]
    got = e.g1_dft(inp)
    ev = NO.ntt(xs)
    for j in sorted({0, 1, 2, m // 2, m - 1} | set(random.Random(m).sample(range(m), 3))):
        assert got[j].compress() == TO.g1_scalar(oracle, ev[j]), j
    back = e.g1_dft(got, inverse=True)
    assert np.array_equal(_stack(back), np.ascontiguousarray(inp, dtype=np.uint64).reshape(-1, 18))


# ---- FK20 against kzg_cells_and_proofs ------------------------------------------------------------------------------------
def _fk20_vs_cells(e, polys, K_, t):
    n = max(len(p) for p in polys)
    c = np.stack([K.scalars_to_limbs(p + [0] * (n - len(p))) if n else np.zeros((0, 4), np.uint64) for p in polys])
    cells, proofs = e.cells_and_proofs_fk20(c, K_, t)
    assert len(proofs) == len(polys)
    for b in range(len(polys)):
        want_cells, want = e.cells_and_proofs_limbs(c[b], K_, t)
        assert np.array_equal(cells[b], want_cells), b
        assert np.array_equal(_stack(proofs[b]), _stack(want)), b
    return cells, proofs


# every l from 1 to 64, N/n in {1, 2, 4}, n up to 4096
@pytest.mark.parametrize("n,N,l", [(4096, 4096, 1), (1024, 2048, 2), (1024, 4096, 4), (2048, 2048, 8), (256, 1024, 16),
                                   (1000, 2048, 32), (4096, 8192, 64), (64, 64, 64), (100, 128, 1), (33, 128, 32)])
def test_fk20_equals_cells(engines, n, N, l):
    e = engines.bench_srs(max(n - l, 1))  # the SRS of exactly n' - l points
    _fk20_vs_cells(e, [_poly(n, n + N + l)], _log(N), _log(l))


@pytest.fixture(scope="module")
def batched():
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(4096)
    e.set_max_batch(128)  # the cells call of the comparisons, as fast as it goes
    yield e
    e.close()


@pytest.mark.parametrize("l", [1, 4, 64])
def test_fk20_batches_of_ragged_polynomials(batched, l):
    """batches of 1, 3 and 64 with a different n' per polynomial: trailing zeros, n' <= l, n' = 0"""
    e = batched
    K_ = 13 if l > 1 else 12
    n = 4096
    rnd = random.Random(l)
    for batch in (1, 3, 64):
        polys = []
        for b in range(batch):
            keep = [n, n // 2 + 3, l, 0, l + 1, 2 * l - 1, rnd.randrange(n + 1)][b % 7]
            polys.append(_poly(keep, 1000 * l + b) + [0] * (n - keep))
        _fk20_vs_cells(e, polys, K_, _log(l))


def test_fk20_short_inputs_and_prepare(engines):
    e = engines.bench_srs(100)
    e.fk20_prepare(100, 3)
    for n in (0, 1, 8, 9, 15):
        _fk20_vs_cells(e, [_poly(n, n)] if n else [[]], 6, 3)
    e.fk20_prepare(5, 3)  # n <= l: nothing to build
    cells, proofs = e.cells_and_proofs_fk20(np.zeros((2, 0, 4), np.uint64), 4, 2)
    assert cells.shape == (2, 16, 4) and not cells.any() and not _stack(proofs[1]).any()


def test_fk20_large_shape_known_secret(engines, oracle):
    """(2^16, 2^17, 64) against [q_j(s)]G and the pairing check"""
    n, K_, t = 1 << 16, 17, 6
    e = engines.bench_srs(n)
    vals = _poly(n, 16)
    c = K.scalars_to_limbs(vals)
    cells, proofs = e.cells_and_proofs_fk20(c, K_, t)
    proofs = proofs[0]
    assert len(proofs) == 2048
    for j in (0, 1, 1234, 2047):
        q = CO.stride_quotient(vals, 64, CO.cell_root(K_, t, j))
        assert proofs[j].compress() == TO.g1_scalar(oracle, CO.poly_eval(q, S)), j
    cm = e.commit_limbs(c)
    g1 = e.srs_read(0, 64)
    g2 = np.stack([K.srs_g2_at(T.BENCH_SECRET_BE, j) for j in range(65)])
    for j in (5, 2000):
        zs = [K.Scalar(z) for z in CO.cell_points(K_, t, j)]
        ys = [K.Scalar.from_limbs(v) for v in cells[0][j * 64:(j + 1) * 64]]
        assert K.verify_points(cm, proofs[j], zs, ys, g1, g2), j


# ---- memory: comb tables streamed per call when they do not fit the budget; cached transforms reused -----------------------
def test_fk20_streamed_tables_equal_cells(monkeypatch):
    """KZG_FK20_TABLE_MB=0: no comb table is kept, every call builds them a chunk of 8192 bases at a time (two chunks or
    more in every shape here); the outputs stay those of kzg_cells_and_proofs"""
    monkeypatch.setenv("KZG_FK20_TABLE_MB", "0")
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(8192)
    try:
        e.set_max_batch(128)
        for n, N, l in ((8192, 8192, 1), (5000, 8192, 4), (8192, 16384, 64)):
            _fk20_vs_cells(e, [_poly(n, n + l)], _log(N), _log(l))
        _fk20_vs_cells(e, [_poly(4096, 1), _poly(1000, 2) + [0] * 3096, _poly(16, 3) + [0] * 4080], 13, 4)
    finally:
        e.close()


def test_fk20_cached_transform_serves_shorter_polynomials(batched):
    """a transform for L = 2^7 (n' = 4096, l = 64) serves n' = 2000 (L = 2^6 would do) without a rebuild"""
    batched.fk20_prepare(4096, 6)
    _fk20_vs_cells(batched, [_poly(2000, 5) + [0] * 2096, _poly(1500, 6) + [0] * 2596], 13, 6)
    _fk20_vs_cells(batched, [_poly(4096, 7)], 13, 6)


def test_fk20_large_polynomial(oracle):
    """n' = 2^20, l = 64: the comb tables would take 128 GiB, so they are streamed; the proofs against [q_j(s)]G"""
    n, K_, t = 1 << 20, 21, 6
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(n)
    try:
        vals = _poly(n, 20)
        cells, proofs = e.cells_and_proofs_fk20(K.scalars_to_limbs(vals), K_, t, cells=False)
        assert cells is None and len(proofs[0]) == 1 << 15
        for j in (3, 31000):
            q = CO.stride_quotient(vals, 64, CO.cell_root(K_, t, j))
            assert proofs[0][j].compress() == TO.g1_scalar(oracle, CO.poly_eval(q, S)), j
    finally:
        e.close()


# ---- errors, SRS replacement, concurrency, multi-device ------------------------------------------------------------------
def test_fk20_errors(engines, eng):
    srs_len, l = 100, 4
    e = engines.bench_srs(srs_len)
    ok = _poly(srs_len + l, 1)
    e.cells_and_proofs_fk20(K.scalars_to_limbs(ok), 8, 2)  # n' - l = srs_len
    bad = np.stack([K.scalars_to_limbs(ok + [0]), K.scalars_to_limbs(_poly(srs_len + l + 1, 1)), K.scalars_to_limbs(ok + [0])])
    with pytest.raises(K.KzgError) as ei:
        e.cells_and_proofs_fk20(bad, 8, 2)
    assert ei.value.status == K.KZG_ERR_DEGREE_TOO_HIGH
    assert b"polynomial 1" in K.load_library().kzg_last_error(e._h)
    c = K.scalars_to_limbs(_poly(64, 2))
    for K_, t, n in ((23, 0, 64), (10, 7, 64), (3, 4, 8), (5, 0, 64)):  # log N, log l > 6, l > N, n > N
        with pytest.raises(K.KzgError) as ei:
            e.cells_and_proofs_fk20(c[:n], K_, t)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG, (K_, t, n)
    lib = K.load_library()
    out = np.zeros((64, 18), np.uint64)
    ptr, optr = c.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert lib.kzg_cells_and_proofs_fk20(e._h, ptr, 64, 1, 64, 8, 2, None, None) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_cells_and_proofs_fk20(e._h, None, 64, 1, 64, 8, 2, None, optr) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_cells_and_proofs_fk20(None, ptr, 64, 1, 64, 8, 2, None, optr) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_cells_and_proofs_fk20(e._h, ptr, 32, 2, 16, 8, 2, None, optr) == K.KZG_ERR_INVALID_ARG  # stride < n
    assert lib.kzg_fk20_prepare(e._h, 64, 7) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_g1_dft(e._h, ptr, 3, 0, optr) == K.KZG_ERR_INVALID_ARG
    with pytest.raises(K.KzgError) as ei:
        eng.cells_and_proofs_fk20(c, 8, 2)
    assert ei.value.status == K.KZG_ERR_NO_SRS
    assert lib.kzg_fk20_prepare(eng._h, 64, 2) == K.KZG_ERR_NO_SRS


def test_fk20_srs_replacement(oracle):
    n, K_, t = 256, 10, 3
    vals = _poly(n, 7)
    c = K.scalars_to_limbs(vals)
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(n)
    try:
        _, first = e.cells_and_proofs_fk20(c, K_, t)
        other = bytes([9] * 32)
        e.srs_generate(other, n)
        _, second = e.cells_and_proofs_fk20(c, K_, t)
        s2 = T.fr_from_be_bytes(other)
        for j in (0, 77):
            q = CO.stride_quotient(vals, 8, CO.cell_root(K_, t, j))
            assert first[0][j].compress() == TO.g1_scalar(oracle, CO.poly_eval(q, S))
            assert second[0][j].compress() == TO.g1_scalar(oracle, CO.poly_eval(q, s2))
        _, want = e.cells_and_proofs_limbs(c, K_, t)
        assert np.array_equal(_stack(second[0]), _stack(want))
    finally:
        e.close()


def test_fk20_concurrency():
    n = 512
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(n)
    try:
        other = K.scalars_to_limbs(_poly(300, 5))
        want_cm = e.commit_limbs(other).compress()
        refs = {}
        for seed, t in ((1, 4), (2, 2)):
            mine = np.stack([K.scalars_to_limbs(_poly(n, seed + b)) for b in range(3)])
            refs[seed] = (mine, t, [e.cells_and_proofs_limbs(mine[b], 10, t) for b in range(3)])
        errors, stop = [], threading.Event()

        def prove(seed):
            try:
                mine, t, ref = refs[seed]
                for _ in range(3):
                    cells, proofs = e.cells_and_proofs_fk20(mine, 10, t)
                    for b in range(3):
                        assert np.array_equal(cells[b], ref[b][0])
                        assert np.array_equal(_stack(proofs[b]), _stack(ref[b][1]))
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


def test_fk20_multi_device_contexts():
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
        rep.fk20_prepare(n, 5)
        cells, got = rep.cells_and_proofs_fk20(c, 11, 5)
        assert np.array_equal(cells[0], want_cells)
        assert np.array_equal(_stack(got[0]), _stack(want))
    finally:
        rep.close()
    rng = K.Engine(devices=[0, 0])
    try:
        rng.srs_generate(T.BENCH_SECRET_BE, n)
        with pytest.raises(K.KzgError) as ei:
            rng.cells_and_proofs_fk20(c, 11, 5)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        assert b"range-split" in K.load_library().kzg_last_error(rng._h)
        with pytest.raises(K.KzgError) as ei:
            rng.fk20_prepare(n, 5)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        pts = rng.srs_read(0, 4)
        assert len(rng.g1_dft(pts)) == 4  # needs no SRS: runs on the first device
    finally:
        rng.close()
