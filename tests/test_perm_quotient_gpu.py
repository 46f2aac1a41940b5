"""GPU: the quotient of a permutation argument -- kzg_coset_extend, kzg_permutation_constraints_coset,
kzg_vanishing_quotient, their device forms and kzg_permutation_quotient.  Every comparison with tests/perm_quotient_oracle.py is
limb for limb; commitments are compared with kzg_commit bit for bit and with the known-secret shortcut of
tests/trapdoor_oracle.py.

TILE is the workgroup tile of k_pq_constraints (one coset point per lane), read from csrc/engine.h.  The transforms take
launch_fr_dft below 2^11 values and launch_ntt from there on (one LDS pass at 2^11, two at 2^12, three at 2^19): sizes on both
sides of each of these."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import bigint_twin as BT
import device_arena as DA
import fr_extremes as FE
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import perm_quotient_oracle as PQ
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu
R = PQ.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = int(re.search(r"constexpr uint32_t kPqTile = (\d+);",
                     open(os.path.join(ROOT, "kzg_poly_commit_exploration_amd", "csrc", "engine.h")).read()).group(1))
S = BT.fr_from_be_bytes(BT.BENCH_SECRET_BE)
ALPHA, BETA, GAMMA = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % R, 0x1F2E3D4C5B6A79881F2E3D4C5B6A7988 % R, 0x123456789ABCDEF0FEDCBA9876543210 % R
SRS = 2048  # the engine of the composite's cases


@pytest.fixture(scope="module")
def eng():
    e = K.Engine(0)  # extension, constraints and the vanishing quotient need no SRS
    yield e
    e.close()


_CACHE = {}  # references computed once, shared and left unchanged


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _rand(n, seed):
    def make():
        rnd = random.Random(1000 * seed + n)
        return [rnd.randrange(R) for _ in range(n)]
    return _memo(("rand", n, seed), make)


def _limbs(cols, stride=None):
    """columns -> (t, stride, 4); the rows past n hold values that are not the columns'"""
    n = len(cols[0])
    stride = n if stride is None else stride
    out = np.empty((len(cols), stride, 4), dtype=np.uint64)
    for j, c in enumerate(cols):
        out[j] = GO.to_limbs(list(c) + [0xBAD + i for i in range(stride - n)])
    return out


def _sc(ks, alpha=ALPHA, beta=BETA, gamma=GAMMA):
    return [K.Scalar(k) for k in ks], K.Scalar(alpha), K.Scalar(beta), K.Scalar(gamma)


def _download(e, dptr, rows):
    got = np.zeros((rows, 4), dtype=np.uint64)
    assert K.load_library().kzg_dev_download(e._h, got.ctypes.data, C.c_void_p(dptr), rows * 32) == 0
    return got


def _remainder(e, call):
    with pytest.raises(K.KzgError) as ei:
        call()
    assert ei.value.status == K.KZG_ERR_REMAINDER, ei.value
    assert b"not divisible" in K.load_library().kzg_last_error(e._h)  # kzg_last_error says what the status means here


# ---- extension -----------------------------------------------------------------------------------------------------------------
def _extension_case(length, log_N, j):
    """(values over the domain, their coefficients, the values on the coset) of column j"""
    def make():
        vals = _rand(length, 10 + j)
        coef = NO.intt(vals)
        return vals, coef, PQ.coset_extend(coef, log_N)
    return _memo(("ext", length, log_N, j), make)


@pytest.mark.parametrize("log_ext", [0, 1, 2, 3])
@pytest.mark.parametrize("length", [1, 2, 4, 1 << 10, 1 << 11, 1 << 12])
def test_extension_sizes_forms_and_strides(eng, length, log_ext):
    log_N = NO.log2_exact(length) + log_ext
    N = 1 << log_N
    cases = [_extension_case(length, log_N, j) for j in range(3)]
    want = np.stack([GO.to_limbs(c[2]) for c in cases])
    if length <= 4:
        assert cases[0][2] == PQ.coset_extend_direct(cases[0][1], log_N)  # the definition
    vals, coefs = [c[0] for c in cases], [c[1] for c in cases]
    assert np.array_equal(eng.coset_extend_limbs(_limbs(vals[:1]), log_N), want[:1])
    stride = length + 5
    assert np.array_equal(eng.coset_extend_limbs(_limbs(vals, stride), log_N, n=length), want)
    assert np.array_equal(eng.coset_extend_limbs(_limbs(coefs, stride), log_N, form=K.KZG_EXTEND_COEFFS, n=length), want)
    assert np.array_equal(eng.coset_extend_limbs(_limbs(coefs[:1]), log_N, form=K.KZG_EXTEND_COEFFS), want[:1])
    d_in, d_out = eng.dev_alloc(3 * stride * 32), eng.dev_alloc(3 * N * 32)
    try:
        for form, cols in ((K.KZG_EXTEND_VALUES, vals), (K.KZG_EXTEND_COEFFS, coefs)):
            eng.dev_upload(d_in, _limbs(cols, stride))
            eng.coset_extend_device(d_in, length, 3, log_N, d_out, form=form, stride=stride)
            assert np.array_equal(_download(eng, d_out, 3 * N).reshape(3, N, 4), want), form
            eng.coset_extend_device(d_in, length, 1, log_N, d_out, form=form)
            assert np.array_equal(_download(eng, d_out, N), want[0]), form
    finally:
        eng.dev_free(d_in)
        eng.dev_free(d_out)


@pytest.mark.parametrize("log_N", [2, 11, 12])
def test_extension_of_coefficients_of_any_length(eng, log_N):
    N = 1 << log_N
    for length in (3, N - 1, N):
        coefs = [_rand(length, 20 + j) for j in range(2)]
        want = np.stack([GO.to_limbs(_memo(("cext", length, log_N, j), lambda: PQ.coset_extend(coefs[j], log_N))) for j in range(2)])
        got = eng.coset_extend_limbs(_limbs(coefs, length + 3), log_N, form=K.KZG_EXTEND_COEFFS, n=length)
        assert np.array_equal(got, want), length


def test_extension_argument_errors(eng):
    lib = K.load_library()
    a, out = np.zeros((64, 4), dtype=np.uint64), np.zeros((64, 4), dtype=np.uint64)
    p = lambda x: x.ctypes.data
    call = lambda **kw: lib.kzg_coset_extend(*[kw.get(k, v) for k, v in (
        ("ctx", eng._h), ("inp", p(a)), ("len", 4), ("batch", 2), ("stride", 4), ("form", K.KZG_EXTEND_VALUES), ("log_out", 3), ("out", p(out)))])
    assert call() == K.KZG_OK
    for kw in ({"ctx": None}, {"inp": None}, {"out": None}, {"len": 0}, {"len": 3}, {"len": 16}, {"batch": 0}, {"stride": 3}, {"form": 2},
               {"log_out": K.KZG_NTT_MAX_LOG + 1}):
        assert call(**kw) == K.KZG_ERR_INVALID_ARG, kw
    assert call(len=3, form=K.KZG_EXTEND_COEFFS) == K.KZG_OK  # coefficients: any length
    d = eng.dev_alloc(64 * 32)
    try:  # the device form: no overlap
        assert lib.kzg_coset_extend_device(eng._h, C.c_void_p(d), 4, 1, 4, 0, 3, C.c_void_p(d + 64)) == K.KZG_ERR_INVALID_ARG
        assert b"overlaps" in lib.kzg_last_error(eng._h)
    finally:
        eng.dev_free(d)


# ---- the vanishing quotient ----------------------------------------------------------------------------------------------------
def _zh_inverses(n, e):
    we = NO.domain_root(NO.log2_exact(e))
    return [pow((pow(7, n, R) * pow(we, k, R) - 1) % R, R - 2, R) for k in range(e)]


@pytest.mark.parametrize("e", [2, 4, 8])
@pytest.mark.parametrize("n", [1, 2, 512, 1024])
def test_vanishing_quotient_returns_the_cofactor_and_flags_the_rest(eng, n, e):
    N = n * e
    log_N = NO.log2_exact(N)

    def make():
        T = _rand(N - n, 30)[:-1] + [1 + _rand(1, 31)[0] % (R - 1)]  # deg T = N - n - 1 exactly
        num = [((T[k - n] if k >= n else 0) - (T[k] if k < N - n else 0)) % R for k in range(N)]
        return T, PQ.coset_extend(num, log_N), PQ.coset_points(log_N)
    T, vals, pts = _memo(("vq", n, e), make)
    want = GO.to_limbs(T)
    assert np.array_equal(eng.vanishing_quotient_limbs(GO.to_limbs(vals), n), want)
    inv = _zh_inverses(n, e)
    divided = [v * inv[i % e] % R for i, v in enumerate(vals)]
    assert np.array_equal(eng.vanishing_quotient_limbs(GO.to_limbs(divided), n, already_divided=True), want)
    with DA.Arena(eng, seed=N) as arena:  # d_out is exactly N - n rows, between guard bands
        d_in = arena.region(N, name="num", data=GO.to_limbs(vals))
        d_out = arena.region(N - n, name="T")
        arena.upload()
        eng.vanishing_quotient_device(d_in.ptr, N, n, d_out.ptr)
        arena.check(outputs={d_out: want})  # T; the input is left as it was; nothing before, between or past them is written
    # one more coefficient at either edge of the flagged range [N - n, N), and Num + 1
    for at in sorted({N - n, N - 1}):
        bad = [(v + 5 * pow(x, at, R)) % R for v, x in zip(vals, pts)]
        _remainder(eng, lambda: eng.vanishing_quotient_limbs(GO.to_limbs(bad), n))
    _remainder(eng, lambda: eng.vanishing_quotient_limbs(GO.to_limbs([(v + 1) % R for v in vals]), n))
    assert np.array_equal(eng.vanishing_quotient_limbs(GO.to_limbs(vals), n), want)  # the context is as good as before


def test_vanishing_quotient_argument_errors(eng):
    lib = K.load_library()
    a, out = np.zeros((64, 4), dtype=np.uint64), np.zeros((64, 4), dtype=np.uint64)
    call = lambda N, n, ctx=eng._h, inp=a.ctypes.data, o=out.ctypes.data: lib.kzg_vanishing_quotient(ctx, inp, N, n, 0, o)
    assert call(8, 2) == K.KZG_OK and call(8, 8) == K.KZG_OK
    for N, n in ((8, 0), (8, 3), (6, 2), (4, 8), (32, 2), (1 << 23, 1 << 22)):
        assert call(N, n) == K.KZG_ERR_INVALID_ARG, (N, n)
    assert call(8, 2, inp=None) == K.KZG_ERR_INVALID_ARG and call(8, 2, o=None) == K.KZG_ERR_INVALID_ARG


# ---- the constraints kernel ----------------------------------------------------------------------------------------------------
def _min_ext(t):
    e = 2
    while e < t + 1:
        e *= 2
    return e


@pytest.mark.parametrize("widest", [False, True])
@pytest.mark.parametrize("t", [1, 2, 3, 7])
def test_constraints_on_the_coset(eng, t, widest):
    e = 8 if widest else _min_ext(t)
    ks = GO.shifts(t)
    for n in sorted({1, 2, 4, max(1, TILE // (2 * e)), TILE // e, 2 * TILE // e}):  # N: 2 .. below, at and above one tile
        N = n * e
        cols = lambda seed: [_rand(N, seed + j) for j in range(t)]
        wires, sigmas, z, gate = cols(40), cols(50), _rand(N, 60), _rand(N, 61)
        for alpha, beta, g in ((ALPHA, BETA, gate), (ALPHA, BETA, None), (0, BETA, gate), (ALPHA, 0, None)):
            want = PQ.constraints_on_coset(wires, sigmas, z, n, ks, alpha, beta, GAMMA, g)
            got = eng.permutation_constraints_coset_limbs(_limbs(wires, N + 3), _limbs(sigmas, N + 3), GO.to_limbs(z), n,
                                                          *_sc(ks, alpha, beta), gate=None if g is None else GO.to_limbs(g), N=N)
            assert np.array_equal(got, GO.to_limbs(want)), (n, alpha, beta, g is None)
        # the rotation wraps at the last e points: z(w x_i) is z at index i + e - N there
        got = GO.from_limbs(eng.permutation_constraints_coset_limbs(_limbs(wires), _limbs(sigmas), GO.to_limbs(z), n, *_sc(ks)))
        pts = PQ.coset_points(NO.log2_exact(N))
        for i in range(N - e, N):
            zi, zr, x = z[i], z[i + e - N], pts[i]
            a, b = zi, zr
            for j in range(t):
                a = a * ((wires[j][i] + BETA * ks[j] % R * x + GAMMA) % R) % R
                b = b * ((wires[j][i] + BETA * sigmas[j][i] + GAMMA) % R) % R
            zh = (pow(x, n, R) - 1) % R
            l0 = zh * pow(n * (x - 1) % R, R - 2, R) % R
            assert got[i] == (ALPHA * (a - b) + ALPHA * ALPHA % R * (zi - 1) % R * l0) % R * pow(zh, R - 2, R) % R, (n, i)
        # columns of all 0 and of all r - 1
        for v in (0, R - 1):
            flat = [[v] * N for _ in range(t)]
            want = PQ.constraints_on_coset(flat, flat, [v] * N, n, ks, ALPHA, BETA, GAMMA, [v] * N)
            got = eng.permutation_constraints_coset_limbs(_limbs(flat), _limbs(flat), GO.to_limbs([v] * N), n, *_sc(ks),
                                                          gate=GO.to_limbs([v] * N))
            assert np.array_equal(got, GO.to_limbs(want)), (n, v)


def test_constraints_device_form_and_extremal_images(eng):
    t, e, n = 3, 4, TILE // 2
    N, stride = n * e, n * e + 7
    ks = GO.shifts(t)
    inv256 = pow(FE.R256, -1, R)
    images = [v * inv256 % R for v in FE.half_values() + FE.digit_extremal()]
    col = lambda off: [images[(5 * i + off) % len(images)] for i in range(N)]
    wires, sigmas, z, gate = [col(j) for j in range(t)], [col(3 + j) for j in range(t)], col(7), col(8)
    want = GO.to_limbs(PQ.constraints_on_coset(wires, sigmas, z, n, ks, ALPHA, BETA, GAMMA, gate))
    bufs = [eng.dev_alloc(t * stride * 32) for _ in range(2)] + [eng.dev_alloc(N * 32) for _ in range(3)]
    try:
        eng.dev_upload(bufs[0], _limbs(wires, stride))
        eng.dev_upload(bufs[1], _limbs(sigmas, stride))
        eng.dev_upload(bufs[2], GO.to_limbs(z))
        eng.dev_upload(bufs[3], GO.to_limbs(gate))
        eng.permutation_constraints_coset_device(bufs[0], bufs[1], bufs[2], n, e, t, *_sc(ks), bufs[4], d_gate=bufs[3], stride=stride)
        assert np.array_equal(_download(eng, bufs[4], N), want)
        with pytest.raises(K.KzgError) as ei:  # the output may overlap no input
            eng.permutation_constraints_coset_device(bufs[0], bufs[1], bufs[2], n, e, t, *_sc(ks), bufs[2], stride=stride)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG and "overlaps" in str(ei.value)
    finally:
        for b in bufs:
            eng.dev_free(b)


def test_constraints_argument_errors(eng):
    lib = K.load_library()
    a, sc = np.zeros((3, 16, 4), dtype=np.uint64), GO.to_limbs([1, 7, 49])
    p = lambda x: x.ctypes.data
    call = lambda **kw: lib.kzg_permutation_constraints_coset(*[kw.get(k, v) for k, v in (
        ("ctx", eng._h), ("wires", p(a)), ("sigmas", p(a)), ("z", p(a)), ("n", 4), ("rot", 4), ("t", 3), ("stride", 16), ("shifts", p(sc)),
        ("alpha", p(sc)), ("beta", p(sc)), ("gamma", p(sc)), ("gate", None), ("out", p(a)))])
    out = np.zeros((16, 4), dtype=np.uint64)
    assert call(out=p(out)) == K.KZG_OK
    for kw in ({"ctx": None}, {"wires": None}, {"sigmas": None}, {"z": None}, {"shifts": None}, {"alpha": None}, {"beta": None},
               {"gamma": None}, {"out": None}, {"n": 3}, {"n": 0}, {"rot": 3}, {"rot": 16}, {"rot": 2}, {"t": 0}, {"t": 8}, {"stride": 15},
               {"n": 1 << 21, "rot": 4, "stride": 1 << 23}):
        assert call(**dict({"out": p(out)}, **kw)) == K.KZG_ERR_INVALID_ARG, kw


# ---- the composite -------------------------------------------------------------------------------------------------------------
def _argument(k, t, seed):
    def make():
        ks = GO.shifts(t)
        wires, sigmas = GO.true_permutation(k, t, ks, seed)
        z, last = PQ.z_of(wires, sigmas, ks, BETA, GAMMA)
        assert last == 1
        return ks, wires, sigmas, z, PQ.quotient(wires, sigmas, z, ks, ALPHA, BETA, GAMMA)
    return _memo(("arg", k, t, seed), make)


def _check_composite(e, oracle, n, log_ext, T, coeffs, points):
    N = n << log_ext
    full = list(T) + [0] * (N - n - len(T))
    assert np.array_equal(coeffs, GO.to_limbs(full) if full else np.zeros((0, 4), dtype=np.uint64))
    assert len(points) == (1 << log_ext) - 1
    for c, point in enumerate(points):
        chunk = full[c * n:(c + 1) * n]
        assert np.array_equal(point.p1, e.commit_limbs(GO.to_limbs(chunk)).p1), c  # bit for bit kzg_commit of the chunk
        assert point.compress() == TO.g1_scalar(oracle, PQ.horner(chunk, S)), c


@pytest.mark.parametrize("n", [1, 4, 256, 2048])
def test_composite_true_permutations(engines, oracle, n):
    t, log_ext = 3, 2
    e = engines.bench_srs(SRS)
    ks, wires, sigmas, z, T = _argument(NO.log2_exact(n), t, 70 + n)
    coeffs, points = e.permutation_quotient(_limbs(wires, n + 3), _limbs(sigmas, n + 3), GO.to_limbs(z), *_sc(ks), log_ext, n=n)
    _check_composite(e, oracle, n, log_ext, T, coeffs, points)


def test_composite_seven_columns(engines, oracle):
    n, t, log_ext = 64, 7, 3
    e = engines.bench_srs(SRS)
    ks, wires, sigmas, z, T = _argument(6, t, 77)
    coeffs, points = e.permutation_quotient(_limbs(wires), _limbs(sigmas), GO.to_limbs(z), *_sc(ks), log_ext)
    _check_composite(e, oracle, n, log_ext, T, coeffs, points)


def test_composite_broken_arguments_gate_term_and_optional_outputs(engines, oracle):
    n, t, log_ext = 256, 3, 2
    N = n << log_ext
    e = engines.bench_srs(SRS)
    ks, wires, sigmas, z, T = _argument(8, t, 70 + n)
    w, s, zl = _limbs(wires), _limbs(sigmas), GO.to_limbs(z)
    ident = GO.identity_sigmas(8, ks)
    j, i = [(j, i) for j in range(t) for i in range(n) if sigmas[j][i] != ident[j][i]][-1]
    bad = [list(c) for c in wires]
    bad[j][i] = (bad[j][i] + 1) % R
    _remainder(e, lambda: e.permutation_quotient(_limbs(bad), s, zl, *_sc(ks), log_ext))
    _remainder(e, lambda: e.permutation_quotient(w, s, GO.to_limbs([v * 5 % R for v in z]), *_sc(ks), log_ext))
    # G = Z_H R adds R to T
    Rc = _rand(n, 80)
    gate = [((Rc[k - n] if n <= k < 2 * n else 0) - (Rc[k] if k < n else 0)) % R for k in range(2 * n)]
    full = list(T) + [0] * (N - n - len(T))
    T1 = [(a + (Rc[k] if k < n else 0)) % R for k, a in enumerate(full)]
    coeffs, points = e.permutation_quotient(w, s, zl, *_sc(ks), log_ext, gate=GO.to_limbs(PQ.coset_extend(gate, NO.log2_exact(N))))
    _check_composite(e, oracle, n, log_ext, T1, coeffs, points)
    # either output may be left out
    want_c, want_p = e.permutation_quotient(w, s, zl, *_sc(ks), log_ext)
    c, p = e.permutation_quotient(w, s, zl, *_sc(ks), log_ext, want_commitments=False)
    assert p is None and np.array_equal(c, want_c)
    c, p = e.permutation_quotient(w, s, zl, *_sc(ks), log_ext, want_coeffs=False)
    assert c is None and [x.compress() for x in p] == [x.compress() for x in want_p]
    c, p = e.permutation_quotient(w, s, zl, *_sc(ks), log_ext, want_coeffs=False, want_commitments=False)  # only the status
    assert c is None and p is None
    # batched MSMs of several chunks per job give the same points
    lib = K.load_library()
    assert lib.kzg_set_max_batch(e._h, 2) == K.KZG_OK
    try:
        c, p = e.permutation_quotient(w, s, zl, *_sc(ks), log_ext)
        assert np.array_equal(c, want_c) and all(np.array_equal(x.p1, y.p1) for x, y in zip(p, want_p))
    finally:
        assert lib.kzg_set_max_batch(e._h, 1) == K.KZG_OK


def test_composite_statuses_and_multi_device_contexts(engines, oracle):
    n, t, log_ext = 256, 3, 2
    ks, wires, sigmas, z, T = _argument(8, t, 70 + n)
    w, s, zl = _limbs(wires), _limbs(sigmas), GO.to_limbs(z)
    want_c, want_p = engines.bench_srs(SRS).permutation_quotient(w, s, zl, *_sc(ks), log_ext)
    bare = K.Engine(0)
    try:
        with pytest.raises(K.KzgError) as ei:
            bare.permutation_quotient(w, s, zl, *_sc(ks), log_ext)
        assert ei.value.status == K.KZG_ERR_NO_SRS
        c, p = bare.permutation_quotient(w, s, zl, *_sc(ks), log_ext, want_commitments=False)  # needs no SRS
        assert np.array_equal(c, want_c)
    finally:
        bare.close()
    short = K.SetupArtifactsGenerator(BT.BENCH_SECRET_BE).take(n // 2)
    try:
        with pytest.raises(K.KzgError) as ei:
            short.permutation_quotient(w, s, zl, *_sc(ks), log_ext)
        assert ei.value.status == K.KZG_ERR_DEGREE_TOO_HIGH
    finally:
        short.close()
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(BT.BENCH_SECRET_BE, n)
        c, p = rep.permutation_quotient(w, s, zl, *_sc(ks), log_ext)
        assert np.array_equal(c, want_c) and [x.compress() for x in p] == [x.compress() for x in want_p]
        ext = rep.coset_extend_limbs(zl.reshape(1, n, 4), 10)  # the calls that need no SRS run on devices[0]
        assert np.array_equal(ext[0], GO.to_limbs(PQ.coset_extend(NO.intt(z), 10)))
    finally:
        rep.close()
    rng = K.Engine(devices=[0, 0])
    try:
        rng.srs_generate(BT.BENCH_SECRET_BE, n)
        with pytest.raises(K.KzgError) as ei:
            rng.permutation_quotient(w, s, zl, *_sc(ks), log_ext)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG and "range-split" in str(ei.value)
        c, p = rng.permutation_quotient(w, s, zl, *_sc(ks), log_ext, want_commitments=False)
        assert np.array_equal(c, want_c)
        full = list(T) + [0] * (3 * n - len(T))  # T's values on the coset are Num / Z_H there
        assert np.array_equal(rng.vanishing_quotient_limbs(GO.to_limbs(PQ.coset_extend(full, 10)), n, already_divided=True),
                              GO.to_limbs(full))
        for call in (lambda: rng.coset_extend_device(1 << 20, 4, 1, 3, 2 << 20),
                     lambda: rng.vanishing_quotient_device(1 << 20, 8, 2, 2 << 20),
                     lambda: rng.permutation_constraints_coset_device(1 << 20, 2 << 20, 3 << 20, 4, 4, 3, *_sc(ks), 4 << 20)):
            with pytest.raises(K.KzgError) as ei:  # the device forms take single-device contexts
                call()
            assert ei.value.status == K.KZG_ERR_INVALID_ARG
    finally:
        rng.close()


def test_composite_argument_errors(engines):
    e = engines.bench_srs(SRS)
    lib = K.load_library()
    n, t = 8, 3
    a, sc = np.zeros((t, n, 4), dtype=np.uint64), GO.to_limbs([1, 7, 49])
    a[:] = GO.to_limbs([1])[0]
    coef, p1s = np.zeros((3 * n, 4), dtype=np.uint64), np.zeros((3, 18), dtype=np.uint64)
    p = lambda x: x.ctypes.data
    call = lambda **kw: lib.kzg_permutation_quotient(*[kw.get(k, v) for k, v in (
        ("ctx", e._h), ("wires", p(a)), ("sigmas", p(a)), ("z", p(a)), ("n", n), ("t", t), ("stride", n), ("shifts", p(sc)),
        ("alpha", p(sc)), ("beta", p(sc)), ("gamma", p(sc)), ("gate", None), ("log_ext", 2), ("coeffs", p(coef)), ("p1s", p(p1s)))])
    for kw in ({"ctx": None}, {"wires": None}, {"sigmas": None}, {"z": None}, {"shifts": None}, {"alpha": None}, {"beta": None},
               {"gamma": None}, {"n": 6}, {"n": 0}, {"n": 1 << 21, "stride": 1 << 21}, {"t": 0}, {"t": 4}, {"log_ext": 4}, {"log_ext": 1},
               {"stride": n - 1}):
        assert call(**kw) == K.KZG_ERR_INVALID_ARG, kw


def test_a_quotient_beside_commitments_in_flight(engines, oracle):
    n = SRS
    e = engines.bench_srs(n)
    slots = e.num_slots()
    polys = [K.scalars_to_limbs(_rand(n, 90 + i)) for i in range(slots - 1)]
    want = [e.commit_limbs(p).compress() for p in polys]
    ks, wires, sigmas, z, T = _argument(8, 3, 70 + 256)
    bufs = [e.dev_alloc(n * 32) for _ in polys]
    try:
        for b, p in zip(bufs, polys):
            e.dev_upload(b, p)
        for i, b in enumerate(bufs):  # every slot but one holds a job
            e.commit_submit(i, b, n)
        coeffs, points = e.permutation_quotient(_limbs(wires), _limbs(sigmas), GO.to_limbs(z), *_sc(ks), 2)
        assert [e.wait(i).compress() for i in range(slots - 1)] == want
        _check_composite(e, oracle, 256, 2, T, coeffs, points)
    finally:
        for b in bufs:
            e.dev_free(b)


# ---- one size whose transforms take three passes -------------------------------------------------------------------------------
def test_three_pass_transforms_checked_at_two_points():
    """n = 2^17, e = 4, t = 3: N = 2^19 is the least size at which ntt_plan has three passes.  z comes from
    kzg_permutation_product, the coefficients the checker evaluates from kzg_ntt."""
    k, t, log_ext = 17, 3, 2
    n = 1 << k
    assert FE.ntt_plan(k + log_ext - 1) != FE.ntt_plan(k + log_ext) and len(FE.ntt_plan(k + log_ext)) == 3 and len(FE.ntt_plan(k + log_ext - 1)) == 2
    e = K.Engine(0)
    try:
        ks = GO.shifts(t)
        wires, sigmas = GO.true_permutation(k, t, ks, 1717)
        w, s = _limbs(wires), _limbs(sigmas)
        z, last = e.permutation_product_limbs(w, s, [K.Scalar(x) for x in ks], K.Scalar(BETA), K.Scalar(GAMMA))
        assert GO.from_limbs(last) == [1]
        coeffs, _ = e.permutation_quotient(w, s, z, *_sc(ks), log_ext, want_commitments=False)
        T = GO.from_limbs(coeffs)
        fc, sc = ([GO.from_limbs(e.intt_limbs(col)) for col in cols] for cols in (w, s))
        zc = GO.from_limbs(e.intt_limbs(z))
        rnd = random.Random(19)
        for _ in range(2):
            assert PQ.check_at(rnd.randrange(R), T, fc, sc, zc, n, ks, ALPHA, BETA, GAMMA)
    finally:
        e.close()


# ---- the C++ example -----------------------------------------------------------------------------------------------------------
def test_example_program_checks_the_identity_at_a_point():
    """examples/perm_quotient.cpp (built by build()): kzg_permutation_commit -> kzg_permutation_quotient -> T(zeta) Z_H(zeta) =
    Num(zeta) by kzg_evaluate, and the chunks' commitments against kzg_commit"""
    import subprocess

    exe = os.path.join(ROOT, "examples", "perm_quotient")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "== Num(zeta)" in out.stdout, (out.stdout, out.stderr)
