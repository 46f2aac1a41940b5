"""GPU: openings at several point sets (kzg_open_sets and friends) against the big-integer restatement
(tests/open_sets_oracle.py: explicit division per set), [v]G of the trapdoor oracle, the commitment to the oracle's quotient, and
the two calls the scheme contains as special cases (kzg_open_points, kzg_open_combined), bit for bit.

The coefficients are made and compared as blst_fr images (what the C-ABI carries): the values and the quotient are linear in
them, so the oracle works on the images directly; only the scalar of a proof takes the factor 2^256 out."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bigint_twin as T
import kzg_poly_commit_exploration_amd as K
import open_combined_oracle as CO
import open_sets_oracle as SO
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu
R = K.R_MODULUS
RINV = CO.RINV
BENCH_S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)
KINDS = ("random", "max", "top")
SHAPES = ("one_point", "sixteen_points", "plonk", "overlapping", "eight_pairs")
# the lane, tile, finish-kernel and scan-tile edges, and n at and below min |S_g|
NS = (1, 2, 3, 17, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 70001)
GRID = [(n, s) for n in NS for s in SHAPES]


def _block(kind, n, t, seed):
    """(t, n, 4) uint64 images and the same as lists of integers"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 64, size=(t, n, 4), dtype=np.uint64)
    a[..., 3] = rng.integers(0, R >> 192, size=(t, n), dtype=np.uint64)  # below r
    if kind == "max":  # every image r - 1
        a[...] = CO.limbs_from_images([R - 1])[0]
    elif kind == "top":  # a single non-zero coefficient, the last one
        a[:, : n - 1] = 0
    return a, [CO.images_from_limbs(a[i]) for i in range(t)]


def _random(seed):
    return int(np.random.default_rng(seed).integers(1, 1 << 62)) * 0x9E3779B97F4A7C15F39CC0605CEDC835 % R


def _special(c, seed):
    """0, 1, r - 1, the 8th root of unity or a random scalar"""
    return (0, 1, R - 1, SO.ROOT8, _random(seed))[c % 5]


def _points(c, seed):
    """sixteen distinct points: the special value of class c first, then its product with the 8th root of unity (PLONK's
    z and z w; for z = 0 the next special value), the other special values, random ones"""
    first = _special(c, seed)
    pts = [first, first * SO.ROOT8 % R]
    for v in [_special(c + k, seed + k) for k in range(1, 5)] + [_random(seed + 100 + k) for k in range(16)]:
        if len(pts) < 16 and v not in pts:
            pts.append(v)
    if pts[1] == pts[0]:  # z = 0
        pts[1] = pts.pop()
        pts.append(_random(seed + 200))
    assert len(set(pts)) == 16
    return pts


def _scalars(sets):
    return [[K.Scalar(z) for z in s] for s in sets]


def _values(rows):
    return [[y * RINV % R for y in row] for row in rows]


def _got(ys):
    return [[y.v for y in row] for row in ys]


@pytest.fixture(scope="module")
def eng():
    e = K.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("n,name", GRID)
def test_hook_elementwise(eng, n, name):
    """kzg_quotient_sets (h, its length, the values) against the oracle; gamma, the points, the strides and the three kinds of
    coefficients rotate over the grid so that every pair of choices of gamma and the first point occurs"""
    idx = GRID.index((n, name))
    kinds = KINDS if n <= 4097 else (KINDS[idx % 3],)  # (the oracle is O(n (t + sum |S_g|)) big-integer steps)
    for kind in kinds:
        c = 3 * idx + KINDS.index(kind)
        gamma, pts, stride = _special(c, c), _points(c // 5, c + 1000), n + 5 * ((c // 25) % 2)
        t, set_of, sets = SO.shape(name, pts)
        a, polys = _block(kind, n, t, c)
        ys, h = eng.quotient_sets_limbs(a, set_of, _scalars(sets), K.Scalar(gamma), stride=stride)
        want = SO.quotient(polys, set_of, sets, gamma)
        assert len(h) == len(want) and len(want) <= max(n - min(len(s) for s in sets), 0), (kind, gamma, stride)
        assert np.array_equal(h, CO.limbs_from_images(want)), (kind, gamma, stride)
        assert _got(ys) == _values(SO.values(polys, set_of, sets)), (kind, gamma, stride)


def test_hook_beyond_the_direct_scan_blocks(eng):
    """more than kPolyDirectBlocks = 1024 scan blocks: the block stage runs as a launch of its own.  Sparse coefficients keep the
    oracle at a few seconds."""
    n, t = (1 << 21) + 2049, 2
    rng = np.random.default_rng(5)
    a = np.zeros((t, n, 4), dtype=np.uint64)
    for i in range(t):
        pos = np.concatenate([rng.integers(0, n, size=300), [0, n - 1]])
        vals = rng.integers(0, 1 << 64, size=(len(pos), 4), dtype=np.uint64)
        vals[:, 3] = rng.integers(0, R >> 192, size=len(pos), dtype=np.uint64)
        a[i, pos] = vals
    polys = [CO.images_from_limbs(a[i]) for i in range(t)]
    pa, pb = _random(6), _random(7)
    set_of, sets, gamma = [0, 1], [[pa], [pb, pa]], _random(8)
    ys, h = eng.quotient_sets_limbs(a, set_of, _scalars(sets), K.Scalar(gamma))
    want = SO.quotient(polys, set_of, sets, gamma)
    assert len(want) == n - 1 and len(h) == n - 1
    assert np.array_equal(h, CO.limbs_from_images(want))
    assert _got(ys) == _values(SO.values(polys, set_of, sets))


# (n, shape, extra stride, class of gamma, class of the first point, kind): the grid above thinned to a dozen
PROOF_CASES = [(2, "one_point", 0, 4, 4, "random"), (3, "plonk", 5, 4, 4, "random"), (17, "sixteen_points", 0, 4, 1, "random"),
               (255, "overlapping", 0, 2, 4, "max"), (256, "eight_pairs", 5, 4, 0, "random"), (257, "sixteen_points", 0, 1, 3, "random"),
               (2047, "plonk", 5, 4, 2, "top"), (2048, "one_point", 0, 3, 4, "random"), (2049, "overlapping", 5, 0, 4, "random"),
               (4097, "eight_pairs", 0, 4, 4, "max"), (4097, "sixteen_points", 5, 4, 1, "top"), (70001, "plonk", 5, 4, 3, "random"),
               (70001, "overlapping", 0, 2, 4, "random")]


@pytest.mark.parametrize("n,name,extra,gc,zc,kind", PROOF_CASES)
def test_proof_bytes(engines, oracle, n, name, extra, gc, zc, kind):
    e = engines.bench_srs(4097 if n <= 4097 else 70001)
    seed = 7 * n + SHAPES.index(name)
    gamma, pts = _special(gc, seed), _points(zc, seed + 1)
    t, set_of, sets = SO.shape(name, pts)
    a, polys = _block(kind, n, t, seed)
    ys, pi = e.open_sets_limbs(a, set_of, _scalars(sets), K.Scalar(gamma), stride=n + extra)
    want_ys = SO.values(polys, set_of, sets)
    assert _got(ys) == _values(want_ys)
    v = SO.proof_scalar(polys, set_of, sets, gamma, BENCH_S)
    want = TO.g1_scalar(oracle, v * RINV % R) if v else CO.INFINITY
    assert pi.compress() == want
    h = SO.quotient(polys, set_of, sets, gamma)
    if h:
        assert np.array_equal(pi.p1, e.commit_limbs(CO.limbs_from_images(h)).p1)  # bit for bit
    else:
        assert pi.is_infinity() and not pi.p1.any()
    if t == 1 and len(sets) == 1:  # a multiproof
        single = e.open_points_limbs(a[0], _scalars(sets)[0], [K.Scalar(y) for y in _values(want_ys)[0]])
        assert np.array_equal(pi.p1, single.p1)
    if len(SO.distinct_points(sets)) == 1:  # a combined opening
        _, combined = e.open_combined_limbs(a, K.Scalar(sets[0][0]), K.Scalar(gamma))
        assert np.array_equal(pi.p1, combined.p1)


def test_special_cases_bit_for_bit(engines):
    """t = 1, m = 1 is kzg_open_points and |T| = 1 is kzg_open_combined, whatever the sizes"""
    e = engines.bench_srs(4097)
    for n, k in ((300, 1), (4097, 2), (2500, 16)):
        a, polys = _block("random", n, 1, n)
        zs = _points(4, n)[:k]
        vals = [K.Scalar(TO.poly_eval(polys[0], z) * RINV % R) for z in zs]
        want = e.open_points_limbs(a[0], [K.Scalar(z) for z in zs], vals)
        ys, pi = e.open_sets_limbs(a, [0], [[K.Scalar(z) for z in zs]], K.Scalar(_random(n + 1)))
        assert _got(ys) == [[y.v for y in vals]] and np.array_equal(pi.p1, want.p1), (n, k)
    for n, t in ((2, 2), (300, 17), (4097, 3)):
        a, polys = _block("random", n, t, n + t)
        z, gamma = K.Scalar(_random(n + 2)), K.Scalar(_random(n + 3))
        want_ys, want = e.open_combined_limbs(a, z, gamma)
        ys, pi = e.open_sets_limbs(a, [0] * t, [[z]], gamma)
        assert _got(ys) == [[y.v] for y in want_ys] and np.array_equal(pi.p1, want.p1), (n, t)


def test_same_bytes_by_every_route(engines, oracle):
    """the host-pointer call at three groupings and the resident submit / wait on a strided block give the same bytes"""
    n = 4097
    e = engines.bench_srs(4097)
    t, set_of, sets = SO.shape("overlapping", _points(4, 11))
    a, polys = _block("random", n, t, 12)
    gamma, zs = K.Scalar(_random(13)), _scalars(sets)
    want_y = _values(SO.values(polys, set_of, sets))
    want_pi = TO.g1_scalar(oracle, SO.proof_scalar(polys, set_of, sets, gamma.v, BENCH_S) * RINV % R)
    got = []
    before = e.max_batch()
    try:
        for mb in (1, 3, t):
            e.set_max_batch(mb)
            ys, pi = e.open_sets_limbs(a, set_of, zs, gamma)
            assert _got(ys) == want_y, mb
            got.append(pi.p1.tobytes())
            hy, h = e.quotient_sets_limbs(a, set_of, zs, gamma, stride=n + 5)
            assert _got(hy) == want_y and np.array_equal(pi.p1, e.commit_limbs(h).p1), mb
    finally:
        e.set_max_batch(before)
    stride = n + 5
    block = np.zeros((t, stride, 4), dtype=np.uint64)
    block[:, :n] = a
    d = e.dev_alloc(block.nbytes)
    try:
        e.dev_upload(d, block)
        e.open_sets_submit(2, d, n, t, set_of, zs, gamma, stride=stride)
        for other in (lambda: e.wait(2), lambda: e.wait_combined(2, t)):  # neither collects it; the job stays in the slot
            with pytest.raises(K.KzgError) as ei:
                other()
            assert ei.value.status == K.KZG_ERR_INVALID_ARG
        ys, pi = e.wait_sets(2, set_of, zs)
        assert _got(ys) == want_y
        got.append(pi.p1.tobytes())
        with pytest.raises(K.KzgError) as ei:  # the slot is idle again
            e.wait_sets(2, set_of, zs)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        # ... and kzg_wait_sets refuses the other kinds, leaving them in their slot
        z = K.Scalar(_random(14))
        e.open_combined_submit(1, d, n, t, z, gamma, stride=stride)
        with pytest.raises(K.KzgError) as ei:
            e.wait_sets(1, set_of, zs)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        e.wait_combined(1, t)
    finally:
        e.dev_free(d)
    assert len(set(got)) == 1 and K.G1Point(np.frombuffer(got[0], dtype=np.uint64)).compress() == want_pi


def test_degree_against_an_srs_of_2048_points(engines, oracle):
    e = engines.bench_srs(2048)
    pts = _points(4, 31)
    set_of, sets = [0, 1, 1], [[pts[0], pts[1]], [pts[2], pts[0], pts[3]]]  # min |S_g| = 2
    gamma = _random(32)
    for n, ok in ((2050, True), (2051, False)):  # n' = n - 2: 2048 fits, 2049 does not
        a, polys = _block("random", n, 3, n)
        if ok:
            ys, pi = e.open_sets_limbs(a, set_of, _scalars(sets), K.Scalar(gamma))
            assert _got(ys) == _values(SO.values(polys, set_of, sets))
            assert pi.compress() == TO.g1_scalar(oracle, SO.proof_scalar(polys, set_of, sets, gamma, BENCH_S) * RINV % R)
        else:
            with pytest.raises(K.KzgError) as ei:
                e.open_sets_limbs(a, set_of, _scalars(sets), K.Scalar(gamma))
            assert ei.value.status == K.KZG_ERR_DEGREE_TOO_HIGH


def test_cancellation_and_gamma_zero(engines, oracle):
    e = engines.bench_srs(4097)
    n = 3000
    a, polys = _block("random", n, 3, 21)
    pts = _points(4, 22)
    sets = [[pts[0], pts[1]], [pts[2]]]
    # two equal polynomials on one set with gamma = r - 1: F_0 = P - P vanishes, the proof is infinity, the values are returned
    both = np.stack([a[0], a[0]])
    ys, pi = e.open_sets_limbs(both, [0, 0], _scalars(sets[:1]), K.Scalar(R - 1))
    row = _values([[TO.poly_eval(polys[0], z) for z in sets[0]]])[0]
    assert _got(ys) == [row, row] and pi.is_infinity() and not pi.p1.any()
    # gamma = 0: the proof of polynomial 0 alone (0^0 = 1), and all values are still returned
    set_of = [1, 0, 1]
    ys, pi = e.open_sets_limbs(a, set_of, _scalars(sets), K.Scalar(0))
    assert _got(ys) == _values(SO.values(polys, set_of, sets))
    alone = e.open_points_limbs(a[0], _scalars(sets)[1], [K.Scalar(TO.poly_eval(polys[0], pts[2]) * RINV % R)])
    assert np.array_equal(pi.p1, alone.p1) and not pi.is_infinity()
    # no coefficients at all: every value is zero, the proof is infinity
    ys, pi = e.open_sets_limbs(np.zeros((3, 0, 4), dtype=np.uint64), set_of, _scalars(sets), K.Scalar(7))
    assert _got(ys) == [[0], [0, 0], [0]] and pi.is_infinity()


def test_argument_errors(engines):
    e = engines.bench_srs(4097)
    lib = K.load_library()
    n, t = 100, 3
    a, _ = _block("random", n, t, 41)
    pts = _points(4, 42)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    u32 = lambda v: np.ascontiguousarray(v, dtype=np.uint32)
    rows = lambda v: np.ascontiguousarray(np.stack([K.Scalar(x).limbs() for x in v]), dtype=np.uint64)
    g = K.Scalar(7).limbs()
    ys, out = np.zeros((K.KZG_MAX_COMBINE * 16 + 16, 4), dtype=np.uint64), np.zeros(18, dtype=np.uint64)
    not_fr = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)

    def call(t=t, stride=n, set_of=(0, 1, 0), sets=((pts[0],), (pts[1], pts[0])), m=None, gamma=g, zs=None, null=None):
        zl = zs if zs is not None else rows([z for s in sets for z in s] or [0])
        args = [e._h, p(a), n, t, stride, p(u32(set_of)), p(u32([len(s) for s in sets])), len(sets) if m is None else m, p(zl),
                p(gamma), p(ys), p(out)]
        if null is not None:
            args[null] = None
        return lib.kzg_open_sets(*args)

    bad = K.KZG_ERR_INVALID_ARG
    assert call() == K.KZG_OK
    assert call(t=0) == bad and call(t=K.KZG_MAX_COMBINE + 1) == bad
    assert call(m=0) == bad and call(m=K.KZG_MAX_SETS + 1) == bad
    assert call(sets=((pts[0],), ())) == bad and b"empty" in lib.kzg_last_error(e._h)
    assert call(set_of=(0, 0, 0)) == bad and b"no polynomial" in lib.kzg_last_error(e._h)
    assert call(set_of=(0, 2, 0)) == bad
    assert call(sets=((pts[0],), (pts[1], pts[1]))) == bad and b"equal points" in lib.kzg_last_error(e._h)
    assert call(sets=(tuple(pts[:9]), tuple(pts[7:16]) + (_random(43),))) == bad and b"distinct points" in lib.kzg_last_error(e._h)
    assert call(sets=(tuple(pts[:8]), tuple(pts[4:16]))) == K.KZG_OK  # sixteen distinct points, some of them in both sets
    zl = rows([pts[0], pts[1], pts[0]])
    zl[1] = not_fr
    assert call(zs=zl) == bad and call(gamma=not_fr) == bad and b"not below r" in lib.kzg_last_error(e._h)
    for pos in (1, 5, 6, 8, 9, 10, 11):
        assert call(null=pos) == bad, pos
    assert call(stride=n - 1) == bad  # stride < n with t > 1
    assert call(t=1, stride=0, set_of=(0,), sets=((pts[0],),)) == K.KZG_OK  # (the stride of one polynomial is not read)
    so, sl, zs1 = u32([0]), u32([1]), rows([pts[0]])
    assert lib.kzg_open_sets_submit(e._h, 0, None, n, 1, n, p(so), p(sl), 1, p(zs1), p(g)) == bad
    hn = ctypes.c_size_t(0)
    assert lib.kzg_quotient_sets(e._h, p(a), n, 0, n, p(so), p(sl), 1, p(zs1), p(g), p(ys), p(ys), ctypes.byref(hn)) == bad


def test_round_trip_commit_open_verify(engines):
    e = engines.bench_srs(4097)
    n = 4000
    for name in ("plonk", "overlapping"):
        t, set_of, sets = SO.shape(name, _points(4, 51))
        a, _ = _block("random", n, t, 52)
        gamma, zs = K.Scalar(_random(53)), _scalars(sets)
        commitments = e.commit_batch_host(a)
        ys, pi = e.open_sets_limbs(a, set_of, zs, gamma)
        g1 = e.srs_read(0, 16)
        g2 = np.stack([K.srs_g2_at(T.BENCH_SECRET_BE, j) for j in range(len(SO.distinct_points(sets)) + 1)])
        assert K.verify_sets(commitments, set_of, zs, ys, gamma, pi, g1, g2)
        bad = [list(row) for row in ys]
        bad[2][0] = K.Scalar(bad[2][0].v + 1)
        assert not K.verify_sets(commitments, set_of, zs, bad, gamma, pi, g1, g2)


def test_multi_device_contexts(oracle):
    n = 3000
    t, set_of, sets = SO.shape("plonk", _points(4, 71))
    a, polys = _block("random", n, t, 72)
    gamma, zs = K.Scalar(_random(73)), _scalars(sets)
    want_y = _values(SO.values(polys, set_of, sets))
    want_pi = TO.g1_scalar(oracle, SO.proof_scalar(polys, set_of, sets, gamma.v, BENCH_S) * RINV % R)
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(T.BENCH_SECRET_BE, n)
        ys, pi = rep.open_sets_limbs(a, set_of, zs, gamma)
        assert _got(ys) == want_y and pi.compress() == want_pi
        assert _got(rep.quotient_sets_limbs(a, set_of, zs, gamma)[0]) == want_y
    finally:
        rep.close()
    rng = K.Engine(devices=[0, 0])
    try:
        rng.srs_generate(T.BENCH_SECRET_BE, n)
        with pytest.raises(K.KzgError) as ei:
            rng.open_sets_limbs(a, set_of, zs, gamma)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        assert b"not supported" in K.load_library().kzg_last_error(rng._h)
    finally:
        rng.close()


def test_example_open_sets_runs():
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "open_sets")
    if not os.path.exists(exe):
        pytest.skip("examples/open_sets is not built")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
