"""GPU: the grand-product entry points -- kzg_grand_product, kzg_permutation_product, their device
forms and kzg_permutation_commit.  Every comparison is exact: through tests/grand_product_oracle.py's inversion-free checker
(z_0 = 1, z_(i+1) B_i = z_i A_i, which has one solution), against the direct definition at n <= 64, limb for limb between the
forms, and for commitments against kzg_commit_lagrange and the known-secret shortcut of tests/trapdoor_oracle.py.

T = 1024 is the tile of k_gp_tile (256 lanes x a run of 4 consecutive indices), L = 256 the lanes of k_gp_carry, each of which
owns ceil(tiles / L) consecutive tiles.  Sizes: below, at and past a run (1 .. 5), around one and two tiles, and
(L + 1) T + 3: more tiles than the carry kernel has lanes (two tiles per lane) with a ragged last tile."""
import ctypes as C
import random

import numpy as np
import pytest

import bigint_twin as BT
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu
R = GO.R
T, L = 1024, 256
S = BT.fr_from_be_bytes(BT.BENCH_SECRET_BE)
ONE = [int(x) for x in GO.to_limbs([1])[0]]
NONE = C.c_size_t(-1).value


@pytest.fixture(scope="module")
def eng():
    e = K.Engine(0)  # the product calls need no SRS
    yield e
    e.close()


_COLS = {}  # (n, t, seed) -> t columns of n non-zero values: computed once, shared and left unchanged


def _cols(n, t, seed):
    if (n, t, seed) not in _COLS:
        rnd = random.Random(1000 * seed + 17 * n + t)
        _COLS[(n, t, seed)] = [[rnd.randrange(1, R) for _ in range(n)] for _ in range(t)]
    return _COLS[(n, t, seed)]


def _limbs(cols, stride=None):
    """t columns -> (t, stride, 4); the rows past n hold values that are not the columns'"""
    n = len(cols[0])
    stride = n if stride is None else stride
    out = np.empty((len(cols), stride, 4), dtype=np.uint64)
    for j, c in enumerate(cols):
        out[j] = GO.to_limbs(list(c) + [0xBAD + i for i in range(stride - n)])
    return out


def _product(eng, nums, dens, stride=None):
    n = len(nums[0])
    z, last = eng.grand_product_limbs(_limbs(nums, stride), _limbs(dens, stride), n=n)
    return GO.from_limbs(z), GO.from_limbs(last)[0]


# ---- the general form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 3, 16])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, T - 1, T, T + 1, 2 * T, 2 * T + 1])
def test_general_form_sizes_and_strides(eng, n, t):
    nums, dens = _cols(n, t, 1), _cols(n, t, 2)
    z, last = _product(eng, nums, dens)
    assert GO.check(nums, dens, z, last)
    if n <= 64:
        assert (z, last) == GO.direct(nums, dens)
    assert _product(eng, nums, dens, stride=n + 5) == (z, last)


def test_more_tiles_than_the_carry_kernel_has_lanes(eng):
    n = (L + 1) * T + 3
    nums, dens = _cols(n, 1, 3), _cols(n, 1, 4)
    z, last = _product(eng, nums, dens)
    assert GO.check(nums, dens, z, last)


@pytest.mark.parametrize("t", [1, 3])
def test_structured_values(eng, t):
    n = 2 * T + 1
    ones = [[1] * n for _ in range(t)]
    z, last = eng.grand_product_limbs(_limbs(ones), _limbs(ones))
    assert all([int(x) for x in row] == ONE for row in z) and [int(x) for x in last] == ONE  # the image of one, limb for limb
    m1 = [[R - 1] * n for _ in range(t)]
    assert _product(eng, m1, m1) == ([1] * n, 1)
    z, last = _product(eng, m1, ones)  # (-1)^(t i)
    assert z == [pow(R - 1, t * i, R) for i in range(n)] and last == pow(R - 1, t * n, R)
    for at in (0, T - 1, T, n - 1):  # a zero numerator is legal: z is zero after it
        nums = [list(c) for c in _cols(n, t, 5)]
        nums[t - 1][at] = 0
        dens = _cols(n, t, 6)
        z, last = _product(eng, nums, dens)
        assert GO.check(nums, dens, z, last) and last == 0 and not any(z[at + 1:]) and all(z[:at + 1]), at


@pytest.mark.parametrize("t", [1, 3])
def test_zero_denominators_are_reported_at_the_least_index(eng, t):
    n = 2 * T + 1
    nums, good = _cols(n, t, 7), _cols(n, t, 8)
    lib = K.load_library()
    cases = [([(at, col)], at) for at in (0, T - 1, T, n - 1) for col in sorted({0, t - 1})]
    cases += [([(T + 7, 0), (5, t - 1)], 5), ([(2 * T, t - 1), (T - 1, 0)], T - 1)]  # two zeros in different tiles
    for zeros, want in cases:
        dens = [list(c) for c in good]
        for at, col in zeros:
            dens[col][at] = 0
        with pytest.raises(K.KzgError) as ei:
            _product(eng, nums, dens)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG and ei.value.bad_index == want, (zeros, ei.value)
        assert "index %d" % want in str(ei.value)
        a, b = _limbs(nums), _limbs(dens)
        z, last = np.zeros((n, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        assert lib.kzg_grand_product(eng._h, a.ctypes.data, b.ctypes.data, n, t, n, z.ctypes.data, last.ctypes.data, None) == \
            K.KZG_ERR_INVALID_ARG  # bad_index may be NULL
    z, last = _product(eng, nums, good)  # the context is as good as before
    assert GO.check(nums, good, z, last)


# ---- the permutation form ------------------------------------------------------------------------------------------------------
BETA, GAMMA = 0x1F2E3D4C5B6A79881F2E3D4C5B6A7988 % R, 0x123456789ABCDEF0FEDCBA9876543210 % R


def _perm(eng, wires, sigmas, ks, beta, gamma):
    z, last = eng.permutation_product_limbs(_limbs(wires), _limbs(sigmas), [K.Scalar(k) for k in ks], K.Scalar(beta), K.Scalar(gamma))
    return z, last


@pytest.mark.parametrize("t", [1, 3, 5])
@pytest.mark.parametrize("n", [1, 2, 4, T, 2 * T])
def test_permutation_form_equals_the_general_form_on_its_columns(eng, n, t):
    k, ks = NO.log2_exact(n), GO.shifts(t)
    wires, sigmas = _cols(n, t, 9), _cols(n, t, 10)
    z, last = _perm(eng, wires, sigmas, ks, BETA, GAMMA)
    a, b = GO.perm_columns(wires, sigmas, ks, BETA, GAMMA)
    gz, glast = eng.grand_product_limbs(_limbs(a), _limbs(b))
    assert np.array_equal(z, gz) and np.array_equal(last, glast)  # limb for limb
    assert GO.check(a, b, GO.from_limbs(z), GO.from_limbs(last)[0])
    # a true permutation closes; one changed wire on a cell it moves does not
    wires, sigmas = GO.true_permutation(k, t, ks, 31 * n + t)
    z, last = _perm(eng, wires, sigmas, ks, BETA, GAMMA)
    a, b = GO.perm_columns(wires, sigmas, ks, BETA, GAMMA)
    assert [int(x) for x in last] == ONE and GO.check(a, b, GO.from_limbs(z), 1)
    ident = GO.identity_sigmas(k, ks)
    moved = [(j, i) for j in range(t) for i in range(n) if sigmas[j][i] != ident[j][i]]
    if moved:
        j, i = moved[-1]
        wires[j][i] = (wires[j][i] + 1) % R
        z, last = _perm(eng, wires, sigmas, ks, BETA, GAMMA)
        a, b = GO.perm_columns(wires, sigmas, ks, BETA, GAMMA)
        assert [int(x) for x in last] != ONE and GO.check(a, b, GO.from_limbs(z), GO.from_limbs(last)[0])
    # beta = 0: numerators and denominators are equal
    z, last = _perm(eng, _cols(n, t, 9), _cols(n, t, 10), ks, 0, GAMMA)
    assert all([int(x) for x in row] == ONE for row in z) and [int(x) for x in last] == ONE


@pytest.mark.parametrize("multiple", [0, 1, 2])
def test_permutation_zero_denominator_whose_sum_is_a_multiple_of_r(eng, multiple):
    """b = f + beta sigma + gamma = 0 with the integer sum of the images of f and gamma and the lazy product beta sigma (the
    representative of -(f + gamma) within +-r/2) at exactly 0, r or 2 r: the images of f and gamma choose the multiple (their
    sum 0.2 r, 1.1 r, 1.85 r), as in tests/test_grand_product.py's replay, which counts them."""
    n, t, at, col = 2 * T, 3, T + 5, 2
    ks = GO.shifts(t)
    inv256 = pow(GO.R256, -1, R)
    gamma_img, f_img = {0: (R // 10, R // 10), 1: (9 * R // 10, R // 5), 2: (9 * R // 10, 19 * R // 20)}[multiple]
    gamma, f = gamma_img * inv256 % R, f_img * inv256 % R
    wires, sigmas = [list(c) for c in _cols(n, t, 11)], [list(c) for c in _cols(n, t, 12)]
    wires[col][at] = f
    sigmas[col][at] = -(f + gamma) * pow(BETA, R - 2, R) % R
    assert GO.first_zero(GO.perm_columns(wires, sigmas, ks, BETA, gamma)[1]) == at
    with pytest.raises(K.KzgError) as ei:
        _perm(eng, wires, sigmas, ks, BETA, gamma)
    assert ei.value.status == K.KZG_ERR_INVALID_ARG and ei.value.bad_index == at, ei.value


# ---- device forms --------------------------------------------------------------------------------------------------------------
def test_device_forms_feed_the_lagrange_commitment(engines, oracle):
    n, t, stride = 2 * T, 3, 2 * T + 5
    e = engines.bench_srs(n)
    e.lagrange_prepare(11)
    lib = K.load_library()
    ks = GO.shifts(t)
    nums, dens = _cols(n, t, 13), _cols(n, t, 14)
    bufs = [e.dev_alloc(t * stride * 32) for _ in range(2)] + [e.dev_alloc(n * 32)]
    try:
        for general in (True, False):
            a, b = _limbs(nums, stride), _limbs(dens, stride)
            e.dev_upload(bufs[0], a)
            e.dev_upload(bufs[1], b)
            if general:
                want_z, want_last = e.grand_product_limbs(a, b, n=n)
                last = e.grand_product_device(bufs[0], bufs[1], n, t, bufs[2], stride=stride)
            else:
                sc = [K.Scalar(k) for k in ks], K.Scalar(BETA), K.Scalar(GAMMA)
                want_z, want_last = e.permutation_product_limbs(a, b, *sc, n=n)
                last = e.permutation_product_device(bufs[0], bufs[1], n, t, *sc, bufs[2], stride=stride)
            got = np.zeros((n, 4), dtype=np.uint64)
            assert lib.kzg_dev_download(e._h, got.ctypes.data, C.c_void_p(bufs[2]), n * 32) == 0
            assert np.array_equal(got, want_z) and np.array_equal(last, want_last)
            e.commit_lagrange_submit(0, bufs[2], n)  # z never visits the host
            point = e.wait(0).compress()
            assert point == e.commit_lagrange_limbs(want_z).compress()
            assert point == TO.g1_scalar(oracle, NO.barycentric_eval(GO.from_limbs(want_z), S))
        # the output may overlap no input; a zero denominator is reported as by the host form
        out, bad = np.zeros(4, dtype=np.uint64), C.c_size_t(0)
        assert lib.kzg_grand_product_device(e._h, C.c_void_p(bufs[0]), C.c_void_p(bufs[1]), n, t, stride, C.c_void_p(bufs[1] + 64),
                                            out.ctypes.data, C.byref(bad)) == K.KZG_ERR_INVALID_ARG
        dens0 = [list(c) for c in dens]
        dens0[1][T] = 0
        e.dev_upload(bufs[1], _limbs(dens0, stride))
        with pytest.raises(K.KzgError) as ei:
            e.grand_product_device(bufs[0], bufs[1], n, t, bufs[2], stride=stride)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG and ei.value.bad_index == T
    finally:
        for b in bufs:
            e.dev_free(b)


# ---- kzg_permutation_commit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, T, 2 * T, 1 << 14])  # the one-launch small MSM and the general MSM path
def test_permutation_commit(engines, oracle, n):
    t = 3
    e = engines.bench_srs(n)
    k, ks = NO.log2_exact(n), GO.shifts(t)
    wires, sigmas = GO.true_permutation(k, t, ks, 77 + n)
    w, s = _limbs(wires), _limbs(sigmas)
    sc = [K.Scalar(x) for x in ks], K.Scalar(BETA), K.Scalar(GAMMA)
    want_z, want_last = e.permutation_product_limbs(w, s, *sc)
    a, b = GO.perm_columns(wires, sigmas, ks, BETA, GAMMA)
    zs = GO.from_limbs(want_z)
    assert GO.check(a, b, zs, 1) and [int(x) for x in want_last] == ONE
    point, z, last = e.permutation_commit(w, s, *sc)
    assert e.lagrange_len() == n  # built on first use
    assert np.array_equal(z, want_z) and np.array_equal(last, want_last)
    assert point.compress() == e.commit_lagrange_limbs(want_z).compress()
    assert point.compress() == TO.g1_scalar(oracle, NO.barycentric_eval(zs, S))
    point2, z2, last2 = e.permutation_commit(w, s, *sc, want_z=False)  # out_z NULL
    assert z2 is None and point2.compress() == point.compress() and np.array_equal(last2, want_last)
    sigmas[1][n - 1] = -(wires[1][n - 1] + GAMMA) * pow(BETA, R - 2, R) % R
    with pytest.raises(K.KzgError) as ei:
        e.permutation_commit(w, _limbs(sigmas), *sc)
    assert ei.value.status == K.KZG_ERR_INVALID_ARG and ei.value.bad_index == n - 1


def test_permutation_commit_statuses_and_multi_device_contexts(engines, oracle):
    n, t = 2 * T, 2
    ks = GO.shifts(t)
    wires, sigmas = GO.true_permutation(11, t, ks, 5)
    w, s = _limbs(wires), _limbs(sigmas)
    sc = [K.Scalar(x) for x in ks], K.Scalar(BETA), K.Scalar(GAMMA)
    bare = K.Engine(0)
    try:
        with pytest.raises(K.KzgError) as ei:
            bare.permutation_commit(w, s, *sc)
        assert ei.value.status == K.KZG_ERR_NO_SRS
    finally:
        bare.close()
    with pytest.raises(K.KzgError) as ei:
        engines.bench_srs(T).permutation_commit(w, s, *sc)
    assert ei.value.status == K.KZG_ERR_DEGREE_TOO_HIGH
    single = engines.bench_srs(n)
    want_point, want_z, want_last = single.permutation_commit(w, s, *sc)
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(BT.BENCH_SECRET_BE, n)
        point, z, last = rep.permutation_commit(w, s, *sc)
        assert point.compress() == want_point.compress() and np.array_equal(z, want_z) and np.array_equal(last, want_last)
        z, last = rep.permutation_product_limbs(w, s, *sc)  # the host forms run on devices[0]
        assert np.array_equal(z, want_z) and np.array_equal(last, want_last)
    finally:
        rep.close()
    rng = K.Engine(devices=[0, 0])
    try:
        rng.srs_generate(BT.BENCH_SECRET_BE, n)
        with pytest.raises(K.KzgError) as ei:
            rng.permutation_commit(w, s, *sc)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG and "range-split" in str(ei.value)
        a, b = GO.perm_columns(wires, sigmas, ks, BETA, GAMMA)
        z, last = rng.grand_product_limbs(_limbs(a), _limbs(b))  # needs no SRS
        assert np.array_equal(z, want_z) and np.array_equal(last, want_last)
        with pytest.raises(K.KzgError) as ei:  # the device forms take single-device contexts
            rng.grand_product_device(1 << 20, 2 << 20, n, t, 3 << 20)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
    finally:
        rng.close()


# ---- arguments -----------------------------------------------------------------------------------------------------------------
def test_argument_errors(eng):
    lib = K.load_library()
    n, t = 8, 2
    a = _limbs(_cols(n, t, 15))
    z, last, bad = np.zeros((n, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64), C.c_size_t(0)
    sh, sc = GO.to_limbs(GO.shifts(t)), GO.to_limbs([BETA])
    p = lambda x: x.ctypes.data
    general = lambda **kw: lib.kzg_grand_product(*[kw.get(k, v) for k, v in (
        ("ctx", eng._h), ("nums", p(a)), ("dens", p(a)), ("n", n), ("t", t), ("stride", n), ("z", p(z)), ("last", p(last)),
        ("bad", C.byref(bad)))])
    perm = lambda **kw: lib.kzg_permutation_product(*[kw.get(k, v) for k, v in (
        ("ctx", eng._h), ("nums", p(a)), ("dens", p(a)), ("n", n), ("t", t), ("stride", n), ("shifts", p(sh)), ("beta", p(sc)),
        ("gamma", p(sc)), ("z", p(z)), ("last", p(last)), ("bad", C.byref(bad)))])
    assert general() == K.KZG_OK and perm() == K.KZG_OK
    for call in (general, perm):
        for kw in ({"ctx": None}, {"nums": None}, {"dens": None}, {"z": None}, {"last": None}, {"t": 0}, {"t": K.KZG_GP_MAX_COLUMNS + 1},
                   {"n": 0}, {"n": (1 << K.KZG_NTT_MAX_LOG) + 1, "stride": 1 << 23}, {"stride": n - 1}):
            assert call(**kw) == K.KZG_ERR_INVALID_ARG, kw
    for kw in ({"shifts": None}, {"beta": None}, {"gamma": None}, {"n": 6}, {"n": 3}):  # the permutation form: n a power of two
        assert perm(**kw) == K.KZG_ERR_INVALID_ARG, kw
    assert general(n=6) == K.KZG_OK  # ... the general form takes any n
    out = np.zeros(18, dtype=np.uint64)
    assert lib.kzg_permutation_commit(eng._h, p(a), p(a), n, t, n, p(sh), p(sc), p(sc), p(z), p(last), None, C.byref(bad)) == \
        K.KZG_ERR_INVALID_ARG
    assert lib.kzg_permutation_commit(eng._h, p(a), p(a), 6, t, n, p(sh), p(sc), p(sc), p(z), p(last), p(out), C.byref(bad)) == \
        K.KZG_ERR_INVALID_ARG


# ---- beside jobs in flight -----------------------------------------------------------------------------------------------------
def test_a_grand_product_beside_commitments_in_flight(engines):
    n = 1 << 14
    e = engines.bench_srs(n)
    slots = e.num_slots()
    rnd = random.Random(99)
    polys = [K.scalars_to_limbs([rnd.randrange(R) for _ in range(n)]) for _ in range(slots - 1)]
    want = [e.commit_limbs(p).compress() for p in polys]
    nums, dens = _cols(2 * T + 1, 2, 16), _cols(2 * T + 1, 2, 17)
    bufs = [e.dev_alloc(n * 32) for _ in polys]
    try:
        for b, p in zip(bufs, polys):
            e.dev_upload(b, p)
        for i, b in enumerate(bufs):  # every slot but one holds a job
            e.commit_submit(i, b, n)
        z, last = _product(e, nums, dens)
        assert [e.wait(i).compress() for i in range(slots - 1)] == want
        assert GO.check(nums, dens, z, last)
    finally:
        for b in bufs:
            e.dev_free(b)
