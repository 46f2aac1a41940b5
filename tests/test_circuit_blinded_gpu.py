"""GPU: zero-knowledge circuit proofs -- kzg_blind_evaluations, kzg_commit_evaluations_blinded,
kzg_circuit_quotient_blinded, kzg_circuit_open_blinded, their _device forms, and the unchanged kzg_circuit_verify on what they return.

Coefficients and evaluations are compared limb for limb with tests/blind_oracle.py; commitments bit for bit with kzg_commit of the
oracle's coefficients and, compressed, with the known-secret shortcut [P(s)]G; the proof bit for bit with kzg_open_sets on the
oracle's padded stack and with [h(s)]G.  With all blinders zero the calls must return what kzg_circuit_quotient / kzg_circuit_open
return: that yardstick owes nothing to the new oracle.

Shapes (n, t, log_ext): (8, 3, 2) the smallest with e = t + 1 (two coefficients checked for zero), 16, 256, one tile of
k_lin_combine (2048), two tiles with e > t + 1 and a short top chunk (4096, t = 2), 31 columns (64, 7, 3); every shape with and
without public inputs, input strides n + 5."""
import ctypes as C

import numpy as np
import pytest

import bigint_twin as BT
import blind_oracle as BO
import circuit_oracle as CO
import device_arena as DA
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import perm_quotient_oracle as PQ
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu
R = PQ.R
S = BT.fr_from_be_bytes(BT.BENCH_SECRET_BE)
ALPHA, BETA, GAMMA = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % R, 0x1F2E3D4C5B6A79881F2E3D4C5B6A7988 % R, 0x123456789ABCDEF0FEDCBA9876543210 % R
ZETA, V = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R, 0x6A09E667F3BCC908B2FB1366EA957D3E3ADEC17512775099DA2F590B0667322A % R
SRS = 4096 + 16
SHAPES = [(8, 3, 2), (16, 3, 2), (256, 3, 2), (2048, 3, 2), (4096, 2, 2), (64, 7, 3)]
# below three rows the tail's index ranges overlap ([0, 3) and [n, n + t + 3)); at n = 1, w = 1: one point, z~ twice in its list
TINY = [(1, 2, 3), (2, 2, 3)]
_CACHE = {}  # references computed once, shared and left unchanged


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _circuit(n, t, with_pi=True):
    def make():
        c = CO.satisfied(NO.log2_exact(n), t, 700 + n + t, with_pi)
        z, last = CO.z_of(c, BETA, GAMMA)
        assert last == 1
        return c, z
    return _memo(("circuit", n, t, with_pi), make)


def _case(n, t, log_ext, with_pi=True, seed=0):
    """the oracle's proof of a satisfied circuit under blinders `seed`"""
    def make():
        c, z = _circuit(n, t, with_pi)
        bl = BO.Blinders.random(t, log_ext, 100 * seed + n + t)
        return bl, BO.proof_case(c, z, log_ext, bl, ALPHA, BETA, GAMMA, ZETA, V, S)
    return _memo(("case", n, t, log_ext, with_pi, seed), make)


def _limbs(cols, stride=None):
    """columns -> (t, stride, 4); the rows past n hold values that are not the columns'"""
    n = len(cols[0])
    stride = n if stride is None else stride
    out = np.empty((len(cols), stride, 4), dtype=np.uint64)
    for j, c in enumerate(cols):
        out[j] = GO.to_limbs(list(c) + [0xBAD + i for i in range(stride - n)])
    return out


def _ch(alpha=ALPHA, beta=BETA, gamma=GAMMA, zeta=ZETA, v=V):
    return [K.Scalar(x) for x in (alpha, beta, gamma, zeta, v)]


def _create(e, c, log_ext, want_key=False):
    return e.circuit_create(_limbs(c.q_lin, c.n + 3), GO.to_limbs(c.q_mul), GO.to_limbs(c.q_const), _limbs(c.sigmas, c.n + 3),
                            [K.Scalar(k) for k in c.ks], log_ext, n=c.n, want_key=want_key)


def _pi(c):
    return None if c.pi is None else GO.to_limbs(c.pi)


def _bl(bl):
    return GO.to_limbs(bl.flat())


def _values(evals):
    abar, sbar, zw = evals
    return [a.v for a in abar], [s.v for s in sbar], zw.v


def _setup(oracle):
    """[s^0]G1 and [s^j]G2, j <= 2, of the bench secret"""
    return _memo("setup", lambda: (np.stack([oracle.p1_generator()]), np.stack([K.srs_g2_at(BT.BENCH_SECRET_BE, j) for j in range(3)])))


def _refused(e, status, call, message=None):
    with pytest.raises(K.KzgError) as ei:
        call()
    assert ei.value.status == status, ei.value
    if message is not None:
        assert message in K.load_library().kzg_last_error(e._h)


def _verify(oracle, circ, c, log_ext, wire_points, z_point, t_points, evals, proof):
    g1, g2 = _setup(oracle)
    public = [] if c.pi is None else [K.Scalar(p) for p in c.pi]
    return K.circuit_verify(circ.key, c.n, log_ext, [K.Scalar(k) for k in c.ks], wire_points, z_point, t_points, public, evals, *_ch(),
                            proof, g1, g2)


# ---- blinded coefficients and their commitments ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,nb", [(1, 1, 3), (2, 1, 3), (1, 2, 2), (8, 3, 2), (16, 1, 3), (2048, 2, 2), (4096, 1, 3), (64, 7, 1)])
def test_blind_evaluations_against_the_oracle(engines, oracle, n, k, nb):
    e = engines.bench_srs(SRS)
    rnd = np.random.default_rng(n + 10 * k + nb)
    cols = [[int.from_bytes(rnd.bytes(32), "little") % R for _ in range(n)] for _ in range(k)]
    b = [[int.from_bytes(rnd.bytes(32), "little") % R for _ in range(nb)] for _ in range(k)]
    want = [BO.blind(NO.intt(col), bj, n) for col, bj in zip(cols, b)]
    evals = _limbs(cols, n + 5)
    got = e.blind_evaluations_limbs(evals, np.stack([GO.to_limbs(bj) for bj in b]), n=n)
    assert got.shape == (k, n + nb, 4)
    for j in range(k):
        assert np.array_equal(got[j], GO.to_limbs(want[j])), j
    # an output stride above n + nb: the rows past n + nb stay the caller's
    out = np.full((k, n + nb + 4, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    bb = np.ascontiguousarray(np.stack([GO.to_limbs(bj) for bj in b]))
    ev = np.ascontiguousarray(evals)
    rc = e._lib.kzg_blind_evaluations(e._h, ev.ctypes.data_as(C.c_void_p), n, k, n + 5, bb.ctypes.data_as(C.c_void_p), nb,
                                      out.ctypes.data_as(C.c_void_p), n + nb + 4)
    assert rc == K.KZG_OK and np.array_equal(out[:, :n + nb], got) and (out[:, n + nb:] == 0x5A5A5A5A5A5A5A5A).all()
    # the commitments: kzg_commit of the oracle's coefficients bit for bit, and [f~(s)]G
    points = e.commit_evaluations_blinded(evals, bb, n=n)
    for j in range(k):
        assert np.array_equal(points[j].p1, e.commit_limbs(GO.to_limbs(want[j])).p1), j
        assert points[j].compress() == TO.g1_scalar(oracle, PQ.horner(want[j], S)), j


def test_blind_evaluations_argument_errors(engines):
    e = engines.bench_srs(SRS)
    n = 8
    evals, b = _limbs([[1] * n]), GO.to_limbs([1, 2, 3]).reshape(1, 3, 4)
    not_fr = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    bad = b.copy()
    bad[0, 2] = not_fr
    _refused(e, K.KZG_ERR_INVALID_ARG, lambda: e.blind_evaluations_limbs(evals, bad), b"is not below r")
    _refused(e, K.KZG_ERR_INVALID_ARG, lambda: e.blind_evaluations_limbs(evals, np.zeros((1, 4, 4), dtype=np.uint64)))  # nb = 4
    _refused(e, K.KZG_ERR_INVALID_ARG, lambda: e.blind_evaluations_limbs(_limbs([[1] * 12]), b))  # n not a power of two
    small = engines.bench_srs(64)
    ev64 = _limbs([[5] * 64])
    _refused(small, K.KZG_ERR_DEGREE_TOO_HIGH, lambda: small.commit_evaluations_blinded(ev64, b))
    assert small.blind_evaluations_limbs(ev64, b).shape == (1, 67, 4)  # needs no SRS of that length
    assert e.blind_evaluations_limbs(evals, b).shape == (1, 11, 4)


# ---- the proof -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t,log_ext,with_pi", [s + (pi,) for pi in (True, False) for s in SHAPES + TINY])
def test_blinded_proof_against_the_oracle_and_the_unchanged_verifier(engines, oracle, n, t, log_ext, with_pi):
    e = engines.bench_srs(SRS)
    bl, d = _case(n, t, log_ext, with_pi)
    c, (key, fw, fz, _) = d["c"], d["coefs"]
    z = _circuit(n, t, with_pi)[1]
    circ = _create(e, c, log_ext, want_key=True)
    try:
        wires, zz, b = _limbs(c.wires, n + 5), GO.to_limbs(z), _bl(bl)
        # round 1 and 2: the wires' and z's commitments
        wire_points = e.commit_evaluations_blinded(wires, b[:2 * t].reshape(t, 2, 4), n=n)
        z_point = e.commit_evaluations_blinded(zz.reshape(1, n, 4), b[2 * t:2 * t + 3].reshape(1, 3, 4))[0]
        for j in range(t):
            assert np.array_equal(wire_points[j].p1, e.commit_limbs(GO.to_limbs(fw[j])).p1), j
            assert wire_points[j].compress() == TO.g1_scalar(oracle, d["wire_s"][j])
        assert z_point.compress() == TO.g1_scalar(oracle, d["z_s"])
        # round 3: T~ limb for limb, its chunks' commitments bit for bit
        t_coeffs, t_points = circ.quotient_blinded(wires, zz, *_ch()[:3], b, public_inputs=_pi(c))
        assert t_coeffs.shape[0] == BO.quotient_len(n, t, log_ext) == circ.blinded_sizes()[1]
        assert np.array_equal(t_coeffs, GO.to_limbs(d["T"]))
        for k, ch in enumerate(d["chunks"]):
            assert np.array_equal(t_points[k].p1, e.commit_limbs(GO.to_limbs(ch)).p1), k
            assert t_points[k].compress() == TO.g1_scalar(oracle, d["t_s"][k]), k
        # rounds 4 and 5: the evaluations limb for limb, the proof bit for bit
        got_evals, proof = circ.open_blinded(wires, zz, t_coeffs, *_ch(), b, public_inputs=_pi(c))
        assert _values(got_evals) == d["evals"]
        ys, want = e.open_sets_limbs([GO.to_limbs(p) for p in d["polys"]], d["set_of"], [[K.Scalar(x) for x in s] for s in d["sets"]],
                                     K.Scalar(V))
        assert np.array_equal(proof.p1, want.p1)
        assert [[y.v for y in row] for row in ys] == d["ys"]
        assert proof.compress() == TO.g1_scalar(oracle, d["w"])
        # the verifier as it is
        assert _verify(oracle, circ, c, log_ext, wire_points, z_point, t_points, got_evals, proof)
        abar, sbar, zw = got_evals
        assert not _verify(oracle, circ, c, log_ext, wire_points, z_point, t_points, (abar, sbar, K.Scalar(zw.v + 1)), proof)
        assert not _verify(oracle, circ, c, log_ext, wire_points, z_point, t_points[::-1], got_evals, proof)
    finally:
        circ.close()


@pytest.mark.parametrize("n,t,log_ext,with_pi", [s + (pi,) for pi in (True, False) for s in SHAPES + TINY])
def test_all_blinders_zero_gives_the_plain_calls(engines, n, t, log_ext, with_pi):
    e = engines.bench_srs(SRS)
    c, z = _circuit(n, t, with_pi)
    N = n << log_ext
    circ = _create(e, c, log_ext)
    try:
        wires, zz, b = _limbs(c.wires, n + 5), GO.to_limbs(z), _bl(BO.Blinders.zero(t, log_ext))
        plain_t, plain_points = circ.quotient(wires, zz, *_ch()[:3], public_inputs=_pi(c))
        plain_evals, plain_proof = circ.open(wires, zz, plain_t, *_ch(), public_inputs=_pi(c))
        t_coeffs, t_points = circ.quotient_blinded(wires, zz, *_ch()[:3], b, public_inputs=_pi(c))
        assert np.array_equal(t_coeffs[:N - n], plain_t) and not t_coeffs[N - n:].any() and t_coeffs.shape[0] == N - n + t + 3
        assert all(np.array_equal(a.p1, p.p1) for a, p in zip(t_points, plain_points))
        got_evals, proof = circ.open_blinded(wires, zz, t_coeffs, *_ch(), b, public_inputs=_pi(c))
        assert _values(got_evals) == _values(plain_evals)
        assert np.array_equal(proof.p1, plain_proof.p1)
        points = e.commit_evaluations_blinded(wires, b[:2 * t].reshape(t, 2, 4), n=n)
        assert all(np.array_equal(points[j].p1, e.commit_evaluations_limbs(GO.to_limbs(c.wires[j])).p1) for j in range(t))
    finally:
        circ.close()


def test_two_blinder_sets_on_one_witness(engines, oracle):
    n, t, log_ext = 256, 3, 2
    e = engines.bench_srs(SRS)
    c, z = _circuit(n, t)
    circ = _create(e, c, log_ext, want_key=True)
    try:
        wires, zz = _limbs(c.wires, n + 5), GO.to_limbs(z)
        runs = []
        for b in (circ.blinders(), circ.blinders()):
            wp = e.commit_evaluations_blinded(wires, b[:2 * t].reshape(t, 2, 4), n=n)
            zp = e.commit_evaluations_blinded(zz.reshape(1, n, 4), b[2 * t:2 * t + 3].reshape(1, 3, 4))[0]
            tc, tp = circ.quotient_blinded(wires, zz, *_ch()[:3], b, public_inputs=_pi(c))
            ev, proof = circ.open_blinded(wires, zz, tc, *_ch(), b, public_inputs=_pi(c))
            assert _verify(oracle, circ, c, log_ext, wp, zp, tp, ev, proof)
            runs.append((wp, zp, tc, tp, ev, proof))
        (wp0, zp0, tc0, tp0, ev0, pr0), (wp1, zp1, tc1, tp1, ev1, pr1) = runs
        assert all(a.compress() != b.compress() for a, b in zip(wp0, wp1)) and zp0.compress() != zp1.compress()
        assert all(a.compress() != b.compress() for a, b in zip(tp0, tp1))
        a0, s0, w0 = _values(ev0)
        a1, s1, w1 = _values(ev1)
        assert all(x != y for x, y in zip(a0, a1)) and w0 != w1 and s0 == s1  # the sigmas are the key's
        assert pr0.compress() != pr1.compress() and not np.array_equal(tc0, tc1)
        # one run's proof does not verify with the other's commitments
        assert not _verify(oracle, circ, c, log_ext, wp1, zp0, tp0, ev0, pr0)
        # what must agree: folded by X^n = 1 every z~ is z's interpolant -- the same values on H, whatever the blinders
        zc = NO.intt(list(z))
        for b in (circ.blinders(), circ.blinders()):
            got = GO.from_limbs(e.blind_evaluations_limbs(zz.reshape(1, n, 4), b[2 * t:2 * t + 3].reshape(1, 3, 4))[0])
            assert [(got[i] + (got[n + i] if i < 3 else 0)) % R for i in range(n)] == zc
    finally:
        circ.close()


# ---- the resident chain, inside guard bands --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t,log_ext", [(8, 3, 2), (256, 3, 2), (64, 7, 3)])
def test_device_chain_inside_guard_bands(engines, oracle, n, t, log_ext):
    e = engines.bench_srs(SRS)
    bl, d = _case(n, t, log_ext)
    c = d["c"]
    LT, stride = BO.quotient_len(n, t, log_ext), n + 5
    circ = _create(e, c, log_ext, want_key=True)
    try:
        with DA.Arena(e, seed=n + t) as arena:
            r_w = arena.region(n, t, stride, "wires", data=_limbs(c.wires))
            r_s = arena.region(n, t, stride, "sigmas", data=_limbs(c.sigmas))
            r_pi = arena.region(n, name="pi", data=_pi(c))
            r_z = arena.region(n, name="z")
            r_t = arena.region(LT + 7, name="T")  # the call is told L_T: the seven rows behind stay fill
            arena.upload()
            last = e.permutation_product_device(r_w.ptr, r_s.ptr, n, t, [K.Scalar(k) for k in c.ks], K.Scalar(BETA), K.Scalar(GAMMA),
                                                r_z.ptr, stride=stride)
            assert K.Scalar.from_limbs(last).v == 1
            t_points = circ.quotient_blinded_device(r_w.ptr, r_z.ptr, *_ch()[:3], _bl(bl), r_t.ptr, d_public_inputs=r_pi.ptr,
                                                    stride=stride)
            evals, proof = circ.open_blinded_device(r_w.ptr, r_z.ptr, r_t.ptr, *_ch(), _bl(bl), d_public_inputs=r_pi.ptr, stride=stride)
            z = _circuit(n, t)[1]
            arena.check({r_z: GO.to_limbs(z), r_t: GO.to_limbs(d["T"])})
        assert _values(evals) == d["evals"]
        assert [p.compress() for p in t_points] == [TO.g1_scalar(oracle, s) for s in d["t_s"]]
        assert proof.compress() == TO.g1_scalar(oracle, d["w"])
        host = circ.open_blinded(_limbs(c.wires), GO.to_limbs(z), GO.to_limbs(d["T"]), *_ch(), _bl(bl), public_inputs=_pi(c))
        assert np.array_equal(host[1].p1, proof.p1) and _values(host[0]) == d["evals"]
    finally:
        circ.close()


# ---- errors, and the context afterwards ----------------------------------------------------------------------------------------
def test_errors_leave_the_context_serving(engines, oracle):
    n, t, log_ext = 256, 3, 2
    e, small = engines.bench_srs(SRS), engines.bench_srs(n + t + 1)
    bl, d = _case(n, t, log_ext)
    c, T = d["c"], d["T"]
    z = _circuit(n, t)[1]
    want = TO.g1_scalar(oracle, d["w"])
    circ, on_small = _create(e, c, log_ext), _create(small, c, log_ext)
    wires, zz, b = _limbs(c.wires), GO.to_limbs(z), _bl(bl)
    try:
        def good():
            got_evals, proof = circ.open_blinded(wires, zz, GO.to_limbs(T), *_ch(), b, public_inputs=_pi(c))
            assert _values(got_evals) == d["evals"] and proof.compress() == want
        good()
        # an unsatisfied gate: the quotient says so
        bad_w = [list(col) for col in c.wires]
        bad_w[0][3] = (bad_w[0][3] + 1) % R
        _refused(e, K.KZG_ERR_REMAINDER, lambda: circ.quotient_blinded(_limbs(bad_w), zz, *_ch()[:3], b, public_inputs=_pi(c)),
                 b"not divisible")
        tc, _ = circ.quotient_blinded(wires, zz, *_ch()[:3], b, public_inputs=_pi(c))
        assert np.array_equal(tc, GO.to_limbs(T))
        # a wrong t_coeffs: a low coefficient, the top one of the last chunk (read by the tail kernel alone)
        for at in (n + 1, t * n + t + 2):
            bad = list(T)
            bad[at] = (bad[at] + 1) % R
            _refused(e, K.KZG_ERR_REMAINDER, lambda: circ.open_blinded(wires, zz, GO.to_limbs(bad), *_ch(), b, public_inputs=_pi(c)),
                     b"does not vanish at zeta")
            good()
        # other blinders than the quotient's
        other = _bl(BO.Blinders.random(t, log_ext, 77))
        _refused(e, K.KZG_ERR_REMAINDER, lambda: circ.open_blinded(wires, zz, GO.to_limbs(T), *_ch(), other, public_inputs=_pi(c)))
        good()
        # a blinder not below r: every group in turn
        not_fr = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
        for row in (0, 2 * t + 2, 2 * t + 3 + (1 << log_ext) - 3):
            bb = b.copy()
            bb[row] = not_fr
            _refused(e, K.KZG_ERR_INVALID_ARG, lambda: circ.quotient_blinded(wires, zz, *_ch()[:3], bb, public_inputs=_pi(c)),
                     b"is not below r")
            _refused(e, K.KZG_ERR_INVALID_ARG, lambda: circ.open_blinded(wires, zz, GO.to_limbs(T), *_ch(), bb, public_inputs=_pi(c)),
                     b"is not below r")
        good()
        # a setup of n + t + 1 points: too short for the opening and for the chunks; the coefficients need none
        _refused(small, K.KZG_ERR_DEGREE_TOO_HIGH, lambda: on_small.open_blinded(wires, zz, GO.to_limbs(T), *_ch(), b, public_inputs=_pi(c)))
        _refused(small, K.KZG_ERR_DEGREE_TOO_HIGH, lambda: on_small.quotient_blinded(wires, zz, *_ch()[:3], b, public_inputs=_pi(c)))
        tc, none = on_small.quotient_blinded(wires, zz, *_ch()[:3], b, public_inputs=_pi(c), want_commitments=False)
        assert none is None and np.array_equal(tc, GO.to_limbs(T))
        good()
    finally:
        circ.close()
        on_small.close()


@pytest.mark.parametrize("n,t,log_ext", [(4, 3, 2), (8, 7, 3)])
def test_shapes_the_rule_refuses(engines, n, t, log_ext):
    e = engines.bench_srs(SRS)
    c, z = _circuit(n, t)
    circ = _create(e, c, log_ext)
    try:
        wires, zz = _limbs(c.wires), GO.to_limbs(z)
        b = np.zeros((2 * t + 3 + (1 << log_ext) - 2, 4), dtype=np.uint64)
        tc = np.zeros((((1 << log_ext) - 1) * n + t + 3, 4), dtype=np.uint64)
        _refused(e, K.KZG_ERR_INVALID_ARG, lambda: circ.quotient_blinded(wires, zz, *_ch()[:3], b, public_inputs=_pi(c)), b"t n + t + 4")
        _refused(e, K.KZG_ERR_INVALID_ARG, lambda: circ.open_blinded(wires, zz, tc, *_ch(), b, public_inputs=_pi(c)), b"t n + t + 4")
        plain_t, _ = circ.quotient(wires, zz, *_ch()[:3], public_inputs=_pi(c), want_commitments=False)  # the plain calls serve
        assert plain_t.shape[0] == (n << log_ext) - n
    finally:
        circ.close()


# ---- contexts over several devices -----------------------------------------------------------------------------------------------
def test_multi_device_contexts(engines, oracle):
    n, t, log_ext = 256, 3, 2
    bl, d = _case(n, t, log_ext)
    c = d["c"]
    z = _circuit(n, t)[1]
    wires, zz, b = _limbs(c.wires), GO.to_limbs(z), _bl(bl)
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(BT.BENCH_SECRET_BE, n + t + 3)
        circ = _create(rep, c, log_ext)
        points = rep.commit_evaluations_blinded(wires, b[:2 * t].reshape(t, 2, 4))
        assert [p.compress() for p in points] == [TO.g1_scalar(oracle, s) for s in d["wire_s"]]
        tc, tp = circ.quotient_blinded(wires, zz, *_ch()[:3], b, public_inputs=_pi(c))  # forwarded to the circuit's device
        assert np.array_equal(tc, GO.to_limbs(d["T"])) and [p.compress() for p in tp] == [TO.g1_scalar(oracle, s) for s in d["t_s"]]
        got_evals, proof = circ.open_blinded(wires, zz, tc, *_ch(), b, public_inputs=_pi(c))
        assert _values(got_evals) == d["evals"] and proof.compress() == TO.g1_scalar(oracle, d["w"])
        _refused(rep, K.KZG_ERR_INVALID_ARG, lambda: circ.open_blinded_device(1 << 20, 2 << 20, 3 << 20, *_ch(), b))  # single-device only
        _refused(rep, K.KZG_ERR_INVALID_ARG, lambda: circ.quotient_blinded_device(1 << 20, 2 << 20, *_ch()[:3], b, 3 << 20))
        circ.close()
    finally:
        rep.close()
    split = K.Engine(devices=[0, 0])
    try:
        split.srs_generate(BT.BENCH_SECRET_BE, n + t + 3)
        circ = _create(split, c, log_ext)
        for call in (lambda: circ.open_blinded(wires, zz, GO.to_limbs(d["T"]), *_ch(), b, public_inputs=_pi(c)),
                     lambda: circ.quotient_blinded(wires, zz, *_ch()[:3], b, public_inputs=_pi(c)),
                     lambda: split.commit_evaluations_blinded(wires, b[:2 * t].reshape(t, 2, 4))):
            with pytest.raises(K.KzgError) as ei:
                call()
            assert ei.value.status == K.KZG_ERR_INVALID_ARG and "range-split" in str(ei.value)
        tc, _ = circ.quotient_blinded(wires, zz, *_ch()[:3], b, public_inputs=_pi(c), want_commitments=False)  # needs no SRS
        assert np.array_equal(tc, GO.to_limbs(d["T"]))
        assert np.array_equal(split.blind_evaluations_limbs(wires, b[:2 * t].reshape(t, 2, 4))[0], GO.to_limbs(d["coefs"][1][0]))
        circ.close()
    finally:
        split.close()
