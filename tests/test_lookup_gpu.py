"""GPU: the log-derivative lookup entry points -- kzg_logderivative_sum, kzg_lookup_sum, their device
forms, kzg_lookup_commit, kzg_batch_inverse and kzg_lookup_multiplicities.  Every comparison is exact: through
tests/lookup_oracle.py's inversion-free checker (phi_0 = 0, (phi_(i+1) - phi_i) D_i = N_i, which has one solution), against the
direct definition at n <= 64, limb for limb between the forms, for commitments against kzg_commit_lagrange and the known-secret
shortcut of tests/trapdoor_oracle.py, and for the multiplicities against the oracle's dict.

T = 512 is the tile of k_lu_tile (256 lanes x a run of R = 2 consecutive rows), L = 256 the lanes of k_lu_carry, each of which
owns ceil(tiles / L) consecutive tiles.  Sizes: below, at and past a run (1 .. 3), around one and two tiles, and (L + 1) T + 3:
more tiles than the carry kernel has lanes (two tiles per lane) with a ragged last tile (t = 1 only: one big-integer pass of
1.3 x 10^5 rows on the Python side)."""
import ctypes as C
import random

import numpy as np
import pytest

import bigint_twin as BT
import kzg_poly_commit_exploration_amd as K
import lookup_oracle as LO
import ntt_oracle as NO
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu
R = LO.R
T, L, RUN = 512, 256, 2
S = BT.fr_from_be_bytes(BT.BENCH_SECRET_BE)
ZERO = [0, 0, 0, 0]
BETA = 0x1F2E3D4C5B6A79881F2E3D4C5B6A7988 % R


@pytest.fixture(scope="module")
def eng():
    e = K.Engine(0)  # the sums, the inverse and the multiplicities need no SRS
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
        out[j] = LO.to_limbs(list(c) + [0xBAD + i for i in range(stride - n)])
    return out


def _sum(eng, nums, dens, stride=None):
    n = len(dens[0])
    phi, last = eng.logderivative_sum_limbs(None if nums is None else _limbs(nums, stride), _limbs(dens, stride), n=n)
    return LO.from_limbs(phi), LO.from_limbs(last)[0]


def _lookup(eng, lookups, table, mult, beta, stride=None):
    n = len(table)
    return eng.lookup_sum_limbs(_limbs(lookups, stride), LO.to_limbs(table), LO.to_limbs(mult), K.Scalar(beta), n=n)


# ---- the general form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 3, 16])
@pytest.mark.parametrize("n", [1, 2, 3, T - 1, T, T + 1, 2 * T, 2 * T + 1])
def test_general_form_sizes_and_strides(eng, n, t):
    nums, dens = _cols(n, t, 1), _cols(n, t, 2)
    phi, last = _sum(eng, nums, dens)
    assert LO.check(nums, dens, phi, last)
    if n <= 64:
        assert (phi, last) == LO.direct(nums, dens)
    assert _sum(eng, nums, dens, stride=n + 5) == (phi, last)


def test_more_tiles_than_the_carry_kernel_has_lanes(eng):
    n = (L + 1) * T + 3
    nums, dens = _cols(n, 1, 3), _cols(n, 1, 4)
    phi, last = _sum(eng, nums, dens)
    assert LO.check(nums, dens, phi, last)


@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("n", [3, 2 * T + 1])
def test_null_numerators_equal_columns_of_ones(eng, n, t):
    dens = _cols(n, t, 5)
    ones = [[1] * n for _ in range(t)]
    phi, last = eng.logderivative_sum_limbs(None, _limbs(dens))
    want_phi, want_last = eng.logderivative_sum_limbs(_limbs(ones), _limbs(dens))
    assert np.array_equal(phi, want_phi) and np.array_equal(last, want_last)  # limb for limb
    assert LO.check(None, dens, LO.from_limbs(phi), LO.from_limbs(last)[0])


@pytest.mark.parametrize("t", [1, 3])
def test_structured_values(eng, t):
    n = 2 * T + 1
    # every fraction is 1: phi_i = t i
    cols = _cols(n, t, 6)
    phi, last = eng.logderivative_sum_limbs(_limbs(cols), _limbs(cols))
    assert [int(x) for x in phi[0]] == ZERO  # the image of zero, limb for limb
    assert LO.from_limbs(phi) == [t * i for i in range(n)] and LO.from_limbs(last)[0] == t * n
    # terms that cancel pairwise: phi is back at 0 at every even row
    nums = [[v if i % 2 == 0 else R - c[i - 1] for i, v in enumerate(c)] for c in cols]
    ones = [[1] * n for _ in range(t)]
    phi, last = _sum(eng, nums, ones)
    assert LO.check(nums, ones, phi, last) and not any(phi[0::2]) and all(phi[1::2])
    for at in (0, RUN - 1, T - 1, T, n - 1):  # a zero numerator is legal
        nums = [list(c) for c in _cols(n, t, 7)]
        nums[t - 1][at] = 0
        dens = _cols(n, t, 8)
        phi, last = _sum(eng, nums, dens)
        assert LO.check(nums, dens, phi, last), at


@pytest.mark.parametrize("t", [1, 3])
def test_zero_denominators_are_reported_at_the_least_row(eng, t):
    n = 2 * T + 1
    nums, good = _cols(n, t, 9), _cols(n, t, 10)
    lib = K.load_library()
    cases = [([(at, col)], at) for at in (0, RUN - 1, RUN, T - 1, T, n - 1) for col in sorted({0, t - 1})]
    cases += [([(T + 7, 0), (5, t - 1)], 5), ([(2 * T, t - 1), (T - 1, 0)], T - 1)]  # two zeros in different tiles
    for zeros, want in cases:
        dens = [list(c) for c in good]
        for at, col in zeros:
            dens[col][at] = 0
        assert LO.first_zero(dens) == want
        with pytest.raises(K.KzgError) as ei:
            _sum(eng, nums, dens)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG and ei.value.bad_index == want, (zeros, ei.value)
        assert "row %d" % want in str(ei.value)
        a, b = _limbs(nums), _limbs(dens)
        phi, last = np.zeros((n, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        assert lib.kzg_logderivative_sum(eng._h, a.ctypes.data, b.ctypes.data, n, t, n, phi.ctypes.data, last.ctypes.data, None) == \
            K.KZG_ERR_INVALID_ARG  # bad_index may be NULL
    phi, last = _sum(eng, nums, good)  # the context is as good as before
    assert LO.check(nums, good, phi, last)


# ---- the lookup form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 15])
@pytest.mark.parametrize("n", [3, 2 * T + 1])
def test_lookup_form_equals_the_general_form_on_its_columns(eng, n, k):
    lookups, table, mult = _cols(n, k, 11), _cols(n, 1, 12)[0], [v % 7 for v in _cols(n, 1, 13)[0]]  # any columns: last != 0
    phi, last = _lookup(eng, lookups, table, mult, BETA)
    a, b = LO.lookup_columns(lookups, table, mult, BETA)
    gphi, glast = eng.logderivative_sum_limbs(_limbs(a), _limbs(b))
    assert np.array_equal(phi, gphi) and np.array_equal(last, glast)  # limb for limb
    assert LO.check(a, b, LO.from_limbs(phi), LO.from_limbs(last)[0])
    phi2, last2 = _lookup(eng, lookups, table, mult, BETA, stride=n + 3)
    assert np.array_equal(phi, phi2) and np.array_equal(last, last2)


@pytest.mark.parametrize("n", [4, T, 2 * T + 1])
def test_a_valid_lookup_closes_and_a_perturbed_one_does_not(eng, n):
    k = 2
    lookups, table, mult = LO.valid_lookup(n, k, 100 + n)
    phi, last = _lookup(eng, lookups, table, mult, BETA)
    a, b = LO.lookup_columns(lookups, table, mult, BETA)
    assert [int(x) for x in last] == ZERO and LO.check(a, b, LO.from_limbs(phi), 0)
    bad = [list(c) for c in lookups]
    bad[1][n - 2] = (bad[1][n - 2] + 1) % R  # one perturbed lookup value
    phi, last = _lookup(eng, bad, table, mult, BETA)
    a, b = LO.lookup_columns(bad, table, mult, BETA)
    assert [int(x) for x in last] != ZERO and LO.check(a, b, LO.from_limbs(phi), LO.from_limbs(last)[0])
    m2 = list(mult)
    m2[n // 2] = (m2[n // 2] + 1) % R  # one perturbed multiplicity
    phi, last = _lookup(eng, lookups, table, m2, BETA)
    a, b = LO.lookup_columns(lookups, table, m2, BETA)
    assert [int(x) for x in last] != ZERO and LO.check(a, b, LO.from_limbs(phi), LO.from_limbs(last)[0])


def test_lookup_zero_denominators(eng):
    n, k = 2 * T + 1, 2
    lookups, table, mult = LO.valid_lookup(n, k, 7)
    for at in (0, T, n - 1):  # beta = -f_0[at]: the least row holding that value is reported
        beta = (R - lookups[0][at]) % R
        want = LO.first_zero(LO.lookup_columns(lookups, table, mult, beta)[1])
        assert want is not None and want <= at
        with pytest.raises(K.KzgError) as ei:
            _lookup(eng, lookups, table, mult, beta)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG and ei.value.bad_index == want, (at, ei.value)
    fresh = _cols(n, k, 14)  # values that occur once: beta = -f_0[i] reports row i, beta = -T_i too
    for col, at in ((0, T - 1), (1, RUN)):
        with pytest.raises(K.KzgError) as ei:
            _lookup(eng, fresh, table, mult, (R - fresh[col][at]) % R)
        assert ei.value.bad_index == at
    tbl = _cols(n, 1, 15)[0]
    with pytest.raises(K.KzgError) as ei:
        _lookup(eng, fresh, tbl, mult, (R - tbl[T]) % R)
    assert ei.value.bad_index == T


# ---- device forms --------------------------------------------------------------------------------------------------------------
def test_device_forms_feed_the_lagrange_commitment(engines, oracle):
    n, k, stride = 2 * T, 2, 2 * T + 5
    t = k + 1
    e = engines.bench_srs(n)
    e.lagrange_prepare(NO.log2_exact(n))
    lib = K.load_library()
    lookups, table, mult = LO.valid_lookup(n, k, 21)
    a, b = LO.lookup_columns(lookups, table, mult, BETA)
    bufs = [e.dev_alloc(t * stride * 32) for _ in range(2)] + [e.dev_alloc(n * 32) for _ in range(3)]
    d_a, d_b, d_out, d_tab, d_m = bufs
    try:
        la, lb = _limbs(a, stride), _limbs(b, stride)
        e.dev_upload(d_a, la)
        e.dev_upload(d_b, lb)
        want_phi, want_last = e.logderivative_sum_limbs(la, lb, n=n)
        got = np.zeros((n, 4), dtype=np.uint64)
        for form in ("general", "lookup", "null"):
            if form == "general":
                last = e.logderivative_sum_device(d_a, d_b, n, t, d_out, stride=stride)
            elif form == "lookup":
                e.dev_upload(d_a, _limbs(lookups, stride))
                e.dev_upload(d_tab, LO.to_limbs(table))
                e.dev_upload(d_m, LO.to_limbs(mult))
                last = e.lookup_sum_device(d_a, n, k, d_tab, d_m, K.Scalar(BETA), d_out, stride=stride)
            else:
                want_phi, want_last = e.logderivative_sum_limbs(None, lb, n=n)
                last = e.logderivative_sum_device(None, d_b, n, t, d_out, stride=stride)
            assert lib.kzg_dev_download(e._h, got.ctypes.data, C.c_void_p(d_out), n * 32) == 0
            assert np.array_equal(got, want_phi) and np.array_equal(last, want_last), form
            e.commit_lagrange_submit(0, d_out, n)  # phi never visits the host
            point = e.wait(0).compress()
            assert point == e.commit_lagrange_limbs(want_phi).compress()
            assert point == TO.g1_scalar(oracle, NO.barycentric_eval(LO.from_limbs(want_phi), S))
        # the batch inverse and the multiplicities on device buffers
        e.dev_upload(d_tab, LO.to_limbs(table))
        e.batch_inverse_device(d_tab, n, d_out)
        assert lib.kzg_dev_download(e._h, got.ctypes.data, C.c_void_p(d_out), n * 32) == 0
        assert np.array_equal(got, e.batch_inverse_limbs(LO.to_limbs(table)))
        d_rows = e.dev_alloc(k * n * 4)
        try:
            e.lookup_multiplicities_device(d_tab, n, d_a, n, k, d_out, d_rows, stride=stride)
            rows = np.zeros((k, n), dtype=np.uint32)
            assert lib.kzg_dev_download(e._h, got.ctypes.data, C.c_void_p(d_out), n * 32) == 0
            assert lib.kzg_dev_download(e._h, rows.ctypes.data, C.c_void_p(d_rows), k * n * 4) == 0
            counts, want_rows, _ = LO.multiplicities(table, lookups)
            assert np.array_equal(got, LO.to_limbs(counts)) and rows.tolist() == want_rows
            bad = C.c_size_t(0)
            assert lib.kzg_lookup_multiplicities_device(e._h, C.c_void_p(d_tab), n, C.c_void_p(d_a), n, k, stride, C.c_void_p(d_a + 32),
                                                        None, C.byref(bad)) == K.KZG_ERR_INVALID_ARG
        finally:
            e.dev_free(d_rows)
        # the output may overlap no input; a zero denominator is reported as by the host form
        out, bad = np.zeros(4, dtype=np.uint64), C.c_size_t(0)
        assert lib.kzg_logderivative_sum_device(e._h, C.c_void_p(d_a), C.c_void_p(d_b), n, t, stride, C.c_void_p(d_b + 64),
                                                out.ctypes.data, C.byref(bad)) == K.KZG_ERR_INVALID_ARG
        bl = K.Scalar(BETA).limbs()
        assert lib.kzg_lookup_sum_device(e._h, C.c_void_p(d_a), n, k, stride, C.c_void_p(d_tab), C.c_void_p(d_m), bl.ctypes.data,
                                         C.c_void_p(d_m), out.ctypes.data, C.byref(bad)) == K.KZG_ERR_INVALID_ARG
        assert lib.kzg_batch_inverse_device(e._h, C.c_void_p(d_tab), n, C.c_void_p(d_tab + 32), C.byref(bad)) == K.KZG_ERR_INVALID_ARG
        b0 = [list(c) for c in b]
        b0[1][T] = 0
        e.dev_upload(d_b, _limbs(b0, stride))
        with pytest.raises(K.KzgError) as ei:
            e.logderivative_sum_device(None, d_b, n, t, d_out, stride=stride)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG and ei.value.bad_index == T
    finally:
        for buf in bufs:
            e.dev_free(buf)


# ---- kzg_lookup_commit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, T, 2 * T, 1 << 14])  # the one-launch small MSM and the general MSM path
def test_lookup_commit(engines, oracle, n):
    k = 2
    e = engines.bench_srs(n)
    lookups, table, mult = LO.valid_lookup(n, k, 77 + n)
    f, tb, m, beta = _limbs(lookups), LO.to_limbs(table), LO.to_limbs(mult), K.Scalar(BETA)
    want_phi, want_last = e.lookup_sum_limbs(f, tb, m, beta)
    a, b = LO.lookup_columns(lookups, table, mult, BETA)
    vals = LO.from_limbs(want_phi)
    assert LO.check(a, b, vals, 0) and [int(x) for x in want_last] == ZERO
    point, phi, last = e.lookup_commit(f, tb, m, beta)
    assert e.lagrange_len() == n  # built on first use
    assert np.array_equal(phi, want_phi) and np.array_equal(last, want_last)
    assert point.compress() == e.commit_lagrange_limbs(want_phi).compress()
    assert point.compress() == TO.g1_scalar(oracle, NO.barycentric_eval(vals, S))
    point2, phi2, last2 = e.lookup_commit(f, tb, m, beta, want_phi=False)  # out_phi NULL
    assert phi2 is None and point2.compress() == point.compress() and np.array_equal(last2, want_last)
    beta0 = (R - table[n - 1]) % R
    with pytest.raises(K.KzgError) as ei:
        e.lookup_commit(f, tb, m, K.Scalar(beta0))
    assert ei.value.status == K.KZG_ERR_INVALID_ARG
    assert ei.value.bad_index == LO.first_zero(LO.lookup_columns(lookups, table, mult, beta0)[1])


def test_lookup_commit_statuses_and_multi_device_contexts(engines):
    n, k = 2 * T, 2
    lookups, table, mult = LO.valid_lookup(n, k, 5)
    f, tb, m, beta = _limbs(lookups), LO.to_limbs(table), LO.to_limbs(mult), K.Scalar(BETA)
    bare = K.Engine(0)
    try:
        with pytest.raises(K.KzgError) as ei:
            bare.lookup_commit(f, tb, m, beta)
        assert ei.value.status == K.KZG_ERR_NO_SRS
    finally:
        bare.close()
    with pytest.raises(K.KzgError) as ei:
        engines.bench_srs(T).lookup_commit(f, tb, m, beta)
    assert ei.value.status == K.KZG_ERR_DEGREE_TOO_HIGH
    single = engines.bench_srs(n)
    with pytest.raises(K.KzgError) as ei:  # n is no power of two
        single.lookup_commit(f, tb, m, beta, n=n - 1)
    assert ei.value.status == K.KZG_ERR_INVALID_ARG
    want_point, want_phi, want_last = single.lookup_commit(f, tb, m, beta)
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(BT.BENCH_SECRET_BE, n)
        point, phi, last = rep.lookup_commit(f, tb, m, beta)
        assert point.compress() == want_point.compress() and np.array_equal(phi, want_phi) and np.array_equal(last, want_last)
        phi, last = rep.lookup_sum_limbs(f, tb, m, beta)  # the host forms run on devices[0]
        assert np.array_equal(phi, want_phi) and np.array_equal(last, want_last)
    finally:
        rep.close()
    rng = K.Engine(devices=[0, 0])
    try:
        rng.srs_generate(BT.BENCH_SECRET_BE, n)
        with pytest.raises(K.KzgError) as ei:
            rng.lookup_commit(f, tb, m, beta)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG and "range-split" in str(ei.value)
        phi, last = rng.lookup_sum_limbs(f, tb, m, beta)  # needs no SRS
        assert np.array_equal(phi, want_phi) and np.array_equal(last, want_last)
        got, _ = rng.lookup_multiplicities(tb, f)
        assert np.array_equal(got, m)
        with pytest.raises(K.KzgError) as ei:  # the device forms take single-device contexts
            rng.logderivative_sum_device(1 << 20, 2 << 20, n, k, 3 << 20)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
    finally:
        rng.close()


def test_a_sum_beside_commitments_in_flight(engines):
    n = 1 << 14
    e = engines.bench_srs(n)
    slots = e.num_slots()
    rnd = random.Random(99)
    polys = [K.scalars_to_limbs([rnd.randrange(R) for _ in range(n)]) for _ in range(slots - 1)]
    want = [e.commit_limbs(p).compress() for p in polys]
    nums, dens = _cols(2 * T + 1, 2, 16), _cols(2 * T + 1, 2, 17)
    lookups, table, mult = LO.valid_lookup(2 * T + 1, 2, 18)
    bufs = [e.dev_alloc(n * 32) for _ in polys]
    try:
        for b, p in zip(bufs, polys):
            e.dev_upload(b, p)
        for i, b in enumerate(bufs):  # every slot but one holds a job
            e.commit_submit(i, b, n)
        phi, last = _sum(e, nums, dens)
        got, _ = e.lookup_multiplicities(LO.to_limbs(table), _limbs(lookups))
        assert [e.wait(i).compress() for i in range(slots - 1)] == want
        assert LO.check(nums, dens, phi, last) and np.array_equal(got, LO.to_limbs(mult))
    finally:
        for b in bufs:
            e.dev_free(b)


# ---- the batch inverse ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, T - 1, T, T + 1, 2 * T, 2 * T + 1, (L + 1) * T + 3])
def test_batch_inverse(eng, n):
    vals = _cols(n, 1, 19)[0]
    out = LO.from_limbs(eng.batch_inverse_limbs(LO.to_limbs(vals)))
    assert all(o * v % R == 1 for o, v in zip(out, vals))


def test_batch_inverse_zeros_and_the_general_form(eng):
    n = 2 * T + 1
    vals = _cols(n, 1, 20)[0]
    inv = eng.batch_inverse_limbs(LO.to_limbs(vals))
    phi, last = eng.logderivative_sum_limbs(None, _limbs([vals]))  # phi_(i+1) - phi_i = 1 / v_i
    sums = LO.from_limbs(phi) + LO.from_limbs(last)
    assert [(b - a) % R for a, b in zip(sums, sums[1:])] == LO.from_limbs(inv)
    for zeros, want in (([0], 0), ([RUN - 1], RUN - 1), ([T - 1], T - 1), ([T], T), ([n - 1], n - 1), ([2 * T, 3], 3)):
        v = list(vals)
        for at in zeros:
            v[at] = 0
        with pytest.raises(K.KzgError) as ei:
            eng.batch_inverse_limbs(LO.to_limbs(v))
        assert ei.value.status == K.KZG_ERR_INVALID_ARG and ei.value.bad_index == want and "row %d" % want in str(ei.value)


# ---- multiplicities ------------------------------------------------------------------------------------------------------------
_TABLES = {}


def _table(n_table, seed=0):
    """distinct random values"""
    if (n_table, seed) not in _TABLES:
        rnd = random.Random(31 * n_table + seed)
        _TABLES[(n_table, seed)] = list({rnd.randrange(R): None for _ in range(n_table + 8)})[:n_table]
    return _TABLES[(n_table, seed)]


def _draw(table, n, k, seed):
    rnd = random.Random(seed)
    return [[table[rnd.randrange(len(table))] for _ in range(n)] for _ in range(k)]


def _mult_matches(eng, table, lookups, log_capacity=None):
    counts, rows, missing = LO.multiplicities(table, lookups)
    assert missing is None
    mult, got_rows = eng.lookup_multiplicities(LO.to_limbs(table), _limbs(lookups), log_capacity=log_capacity)
    assert np.array_equal(mult, LO.to_limbs(counts))
    assert got_rows.tolist() == rows
    return mult


@pytest.mark.parametrize("n,k", [(1, 1), (257, 3), (1 << 14, 2)])
@pytest.mark.parametrize("n_table", [1, 2, 255, 256, 257, 1 << 14])
def test_multiplicities_sizes(eng, n_table, n, k):
    table = _table(n_table)
    lookups = _draw(table, n, k, n_table + n)
    _mult_matches(eng, table, lookups)
    if n == 257:  # a stride past n, and no out_rows
        mult, rows = eng.lookup_multiplicities(LO.to_limbs(table), _limbs(lookups, n + 3), n=n, want_rows=False)
        assert rows is None and np.array_equal(mult, LO.to_limbs(LO.multiplicities(table, lookups)[0]))


def test_multiplicities_hot_row_duplicates_and_structured_tables(eng):
    n, k = 2 * T + 1, 2
    table = _table(300)
    mult = _mult_matches(eng, table, [[table[77]] * n for _ in range(k)])  # every lookup on ONE row
    assert LO.from_limbs(mult[77])[0] == k * n
    same = [table[3]] * 300  # every row equal: all counts at row 0
    mult = _mult_matches(eng, same, [[table[3]] * n for _ in range(k)])
    assert LO.from_limbs(mult)[0] == k * n and not any(LO.from_limbs(mult)[1:])
    twice = table[:150] + table[:150]  # each value twice: counts at the lesser row, 0 at the other
    mult = _mult_matches(eng, twice, _draw(table[:150], n, k, 1))
    assert not any(LO.from_limbs(mult)[150:])
    inv256 = pow(LO.GO.R256, -1, R)
    small = [i * inv256 % R for i in range(1 << 12)]  # the IMAGES are the consecutive integers 0, 1, 2, ..
    assert [int(x) for x in LO.to_limbs(small[:3])[2]] == [2, 0, 0, 0]
    _mult_matches(eng, small, _draw(small, n, k, 2))


@pytest.mark.parametrize("n_table", [256, 1 << 12])
def test_multiplicities_at_load_factor_one(eng, n_table):
    """2^log_capacity = n_table: every slot ends occupied, the walks wrap round the end of the table and chains are long"""
    table = _table(n_table)
    lg = n_table.bit_length() - 1
    lookups = [list(table), _draw(table, n_table, 1, 3)[0]]  # every row is looked up
    _mult_matches(eng, table, lookups, log_capacity=lg)
    missing = [list(c) for c in lookups]
    missing[1][n_table // 2] = _table(n_table, 1)[0]  # in a FULL table a miss ends by the loop bound, not by an empty slot
    assert LO.multiplicities(table, missing)[2] == n_table // 2
    with pytest.raises(K.KzgError) as ei:
        eng.lookup_multiplicities(LO.to_limbs(table), _limbs(missing), log_capacity=lg)
    assert ei.value.status == K.KZG_ERR_INVALID_ARG and ei.value.bad_index == n_table // 2


def test_missing_values_are_reported_at_the_least_row(eng):
    n, k = 2 * T + 1, 3
    table = _table(257)
    other = _table(257, 1)
    lookups = _draw(table, n, k, 4)
    for places, want in (([(0, 0)], 0), ([(1, T)], T), ([(k - 1, n - 1)], n - 1), ([(0, 2 * T), (2, 9)], 9)):
        bad = [list(c) for c in lookups]
        for idx, (col, at) in enumerate(places):
            bad[col][at] = other[idx]
        assert LO.multiplicities(table, bad)[2] == want
        with pytest.raises(K.KzgError) as ei:
            eng.lookup_multiplicities(LO.to_limbs(table), _limbs(bad))
        assert ei.value.status == K.KZG_ERR_INVALID_ARG and ei.value.bad_index == want and "row %d" % want in str(ei.value)
    _mult_matches(eng, table, lookups)  # the context is as good as before


def test_multiplicities_feed_the_lookup_sum(eng):
    n, k = 2 * T + 1, 3
    lookups, table, _ = LO.valid_lookup(n, k, 55)
    mult, _ = eng.lookup_multiplicities(LO.to_limbs(table), _limbs(lookups), want_rows=False)
    phi, last = eng.lookup_sum_limbs(_limbs(lookups), LO.to_limbs(table), mult, K.Scalar(BETA))
    assert [int(x) for x in last] == ZERO and [int(x) for x in phi[0]] == ZERO


# ---- arguments -----------------------------------------------------------------------------------------------------------------
def test_argument_errors(eng):
    lib = K.load_library()
    n, t = 8, 2
    a = _limbs(_cols(n, t, 22))
    phi, last, bad = np.zeros((n, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64), C.c_size_t(0)
    rows = np.zeros((t, n), dtype=np.uint32)
    sc = LO.to_limbs([BETA])
    p = lambda x: x.ctypes.data
    big = (1 << K.KZG_NTT_MAX_LOG) + 1
    general = lambda **kw: lib.kzg_logderivative_sum(*[kw.get(k, v) for k, v in (
        ("ctx", eng._h), ("nums", p(a)), ("dens", p(a)), ("n", n), ("t", t), ("stride", n), ("phi", p(phi)), ("last", p(last)),
        ("bad", C.byref(bad)))])
    lookup = lambda **kw: lib.kzg_lookup_sum(*[kw.get(k, v) for k, v in (
        ("ctx", eng._h), ("lookups", p(a)), ("n", n), ("t", t), ("stride", n), ("table", p(a)), ("mult", p(a)), ("beta", p(sc)),
        ("phi", p(phi)), ("last", p(last)), ("bad", C.byref(bad)))])
    both = np.ascontiguousarray(np.stack([a[0], a[0]]))  # lookup columns whose values are the table's
    mults = lambda **kw: lib.kzg_lookup_multiplicities_cap(*[kw.get(k, v) for k, v in (
        ("ctx", eng._h), ("table", p(a)), ("n_table", n), ("lookups", p(both)), ("n", n), ("t", t), ("stride", n), ("mult", p(phi)),
        ("rows", p(rows)), ("bad", C.byref(bad)), ("cap", 4))])
    assert general() == K.KZG_OK and lookup() == K.KZG_OK and general(nums=None) == K.KZG_OK and general(n=6) == K.KZG_OK
    assert mults() == K.KZG_OK and mults(rows=None) == K.KZG_OK and mults(cap=3) == K.KZG_OK
    for kw in ({"ctx": None}, {"dens": None}, {"phi": None}, {"last": None}, {"t": 0}, {"t": K.KZG_LOGUP_MAX_COLUMNS + 1}, {"n": 0},
               {"n": big, "stride": 1 << 23}, {"stride": n - 1}):
        assert general(**kw) == K.KZG_ERR_INVALID_ARG, kw
    for kw in ({"ctx": None}, {"lookups": None}, {"table": None}, {"mult": None}, {"beta": None}, {"phi": None}, {"last": None}, {"t": 0},
               {"t": K.KZG_LOGUP_MAX_COLUMNS}, {"n": 0}, {"n": big, "stride": 1 << 23}, {"stride": n - 1}):
        assert lookup(**kw) == K.KZG_ERR_INVALID_ARG, kw
    for kw in ({"ctx": None}, {"table": None}, {"lookups": None}, {"mult": None}, {"n_table": 0}, {"t": 0}, {"t": 16}, {"n": 0},
               {"cap": 2}, {"cap": K.KZG_NTT_MAX_LOG + 2}, {"n_table": big, "cap": 23}, {"n": big, "stride": 1 << 23}, {"stride": n - 1}):
        assert mults(**kw) == K.KZG_ERR_INVALID_ARG, kw
    assert lib.kzg_lookup_multiplicities(eng._h, p(a), n, p(both), n, t, n, p(phi), None, C.byref(bad)) == K.KZG_OK
    assert lib.kzg_lookup_multiplicities(eng._h, p(a), 0, p(both), n, t, n, p(phi), None, C.byref(bad)) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_lookup_multiplicities(eng._h, p(a), big, p(both), n, t, n, p(phi), None, C.byref(bad)) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_batch_inverse(eng._h, p(a), n, p(phi), None) == K.KZG_OK
    for args in ((None, p(a), n, p(phi)), (eng._h, None, n, p(phi)), (eng._h, p(a), n, None), (eng._h, p(a), 0, p(phi)),
                 (eng._h, p(a), big, p(phi))):
        assert lib.kzg_batch_inverse(*args, C.byref(bad)) == K.KZG_ERR_INVALID_ARG, args
    out = np.zeros(18, dtype=np.uint64)
    commit = lambda nn, o: lib.kzg_lookup_commit(eng._h, p(a), nn, t, n, p(a), p(a), p(sc), p(phi), p(last), o, C.byref(bad))
    assert commit(n, None) == K.KZG_ERR_INVALID_ARG and commit(6, p(out)) == K.KZG_ERR_INVALID_ARG
    assert commit(n, p(out)) == K.KZG_ERR_NO_SRS
