"""GPU: the last round of a circuit's proof -- kzg_circuit_linearise, kzg_circuit_open,
kzg_circuit_open_device and kzg_circuit_verify on what they return.

r and the evaluations are compared limb for limb with tests/linearise_oracle.py; the proof bit for bit with kzg_open_sets on the
oracle's stack and, compressed, with the known-secret shortcut [h(s)]G of tests/open_sets_oracle.py; the verifier gets the key of
kzg_circuit_create and the commitments of kzg_circuit_quotient, kzg_permutation_commit and kzg_commit_evaluations.

Shapes (n, t, log_ext): n = 1 (zeta w = zeta: one point), small sizes, one full tile of k_lin_combine (2048), two tiles (4096: the
finish kernel sums across tiles), t = 7 with e = 8 (31 columns in the launch for zeta) and the same at n = 1 (32 columns, the
table's maximum); every shape with and without public inputs, input strides n + 5."""
import ctypes as C

import numpy as np
import pytest

import bigint_twin as BT
import circuit_oracle as CO
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import linearise_oracle as LO
import ntt_oracle as NO
import open_sets_oracle as SO
import perm_quotient_oracle as PQ
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu
R = PQ.R
S = BT.fr_from_be_bytes(BT.BENCH_SECRET_BE)
ALPHA, BETA, GAMMA = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % R, 0x1F2E3D4C5B6A79881F2E3D4C5B6A7988 % R, 0x123456789ABCDEF0FEDCBA9876543210 % R
ZETA, V = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R, 0x6A09E667F3BCC908B2FB1366EA957D3E3ADEC17512775099DA2F590B0667322A % R
SRS = 4096
SHAPES = [(1, 3, 2), (2, 3, 2), (4, 3, 2), (256, 3, 2), (2048, 3, 2), (4096, 2, 2), (64, 7, 3), (1, 7, 3)]
_CACHE = {}  # references computed once, shared and left unchanged


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _case(n, t, with_pi=True):
    """(circuit, z, T, coefficient vectors) of a satisfied circuit"""
    def make():
        c = CO.satisfied(NO.log2_exact(n), t, 500 + n + t, with_pi)
        z, last = CO.z_of(c, BETA, GAMMA)
        assert last == 1
        return c, z, CO.quotient(c, z, ALPHA, BETA, GAMMA), LO.coefficients(c, z)
    return _memo(("case", n, t, with_pi), make)


def _lin(n, t, log_ext, with_pi=True, zeta=ZETA):
    """(r, (abar, sbar, zw), the stack) at zeta"""
    def make():
        c, z, T, coefs = _case(n, t, with_pi)
        r = LO.linearisation(c, coefs, T, log_ext, ALPHA, BETA, GAMMA, zeta)
        assert PQ.horner(r, zeta) == 0
        return r, LO.evaluations(c, coefs, zeta), LO.stack(c, coefs, r, zeta)
    return _memo(("lin", n, t, log_ext, with_pi, zeta), make)


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


def _t_limbs(T, n, log_ext):
    return GO.to_limbs([v for ch in LO.chunks(T, n, log_ext) for v in ch])


def _values(evals):
    abar, sbar, zw = evals
    return [a.v for a in abar], [s.v for s in sbar], zw.v


def _open(circ, c, z, T, log_ext, stride=None, **ch):
    return circ.open(_limbs(c.wires, stride), GO.to_limbs(z), _t_limbs(T, c.n, log_ext), *_ch(**ch), public_inputs=_pi(c))


def _setup(oracle):
    """[s^0]G1 and [s^j]G2, j <= 2, of the bench secret"""
    return _memo("setup", lambda: (np.stack([oracle.p1_generator()]), np.stack([K.srs_g2_at(BT.BENCH_SECRET_BE, j) for j in range(3)])))


def _stack_limbs(stack):
    polys, set_of, sets, ys = stack
    return [GO.to_limbs(p) for p in polys], set_of, [[K.Scalar(x) for x in s] for s in sets]


# ---- the linearisation polynomial, limb for limb -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t,log_ext,with_pi", [s + (pi,) for pi in (True, False) for s in SHAPES])
def test_linearise_against_the_oracle(engines, n, t, log_ext, with_pi):
    e = engines.bench_srs(SRS)
    c, z, T, coefs = _case(n, t, with_pi)
    r, evals, _ = _lin(n, t, log_ext, with_pi)
    circ = _create(e, c, log_ext)
    try:
        got_evals, got_r = circ.linearise(_limbs(c.wires, n + 5), GO.to_limbs(z), _t_limbs(T, n, log_ext), *_ch()[:4], public_inputs=_pi(c))
        assert _values(got_evals) == evals
        assert np.array_equal(got_r, GO.to_limbs(r))
    finally:
        circ.close()


# ---- the proof -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t,log_ext,with_pi", [s + (pi,) for pi in (True, False) for s in SHAPES])
def test_open_is_open_sets_of_the_stack_and_verifies(engines, oracle, n, t, log_ext, with_pi):
    e = engines.bench_srs(SRS)
    c, z, T, coefs = _case(n, t, with_pi)
    r, evals, stack = _lin(n, t, log_ext, with_pi)
    circ = _create(e, c, log_ext, want_key=True)
    try:
        wires = _limbs(c.wires, n + 5)
        t_coeffs, t_points = circ.quotient(wires, GO.to_limbs(z), *_ch()[:3], public_inputs=_pi(c))
        assert np.array_equal(t_coeffs, _t_limbs(T, n, log_ext))
        got_evals, proof = circ.open(wires, GO.to_limbs(z), t_coeffs, *_ch(), public_inputs=_pi(c))
        assert _values(got_evals) == evals
        polys, set_of, sets = _stack_limbs(stack)
        ys, want = e.open_sets_limbs(polys, set_of, sets, K.Scalar(V))
        assert np.array_equal(proof.p1, want.p1)  # bit for bit
        assert [[y.v for y in row] for row in ys] == stack[3]
        assert proof.compress() == TO.g1_scalar(oracle, SO.proof_scalar(stack[0], stack[1], stack[2], V, S))
        # the verifier, on what the library's own calls committed to
        wire_points = [e.commit_evaluations_limbs(GO.to_limbs(col)) for col in c.wires]
        z_point, _, _ = e.permutation_commit(_limbs(c.wires), _limbs(c.sigmas), [K.Scalar(k) for k in c.ks], K.Scalar(BETA),
                                             K.Scalar(GAMMA), want_z=False)
        g1, g2 = _setup(oracle)
        public = [] if c.pi is None else [K.Scalar(p) for p in c.pi]
        args = lambda ev, pr: (circ.key, n, log_ext, [K.Scalar(k) for k in c.ks], wire_points, z_point, t_points, public, ev) + \
            tuple(_ch()) + (pr, g1, g2)
        assert K.circuit_verify(*args(got_evals, proof))
        abar, sbar, zw = got_evals
        assert not K.circuit_verify(*args((abar, sbar, K.Scalar(zw.v + 1)), proof))
        assert not K.circuit_verify(*args(got_evals, circ.key[0]))
    finally:
        circ.close()


@pytest.mark.parametrize("which", ["one", "root"])
def test_zeta_inside_the_domain(engines, oracle, which):
    n, t, log_ext = 256, 3, 2
    zeta = 1 if which == "one" else NO.domain_root(8)
    e = engines.bench_srs(SRS)
    c, z, T, coefs = _case(n, t)
    r, evals, stack = _lin(n, t, log_ext, True, zeta)
    circ = _create(e, c, log_ext)
    try:
        got_evals, got_r = circ.linearise(_limbs(c.wires), GO.to_limbs(z), _t_limbs(T, n, log_ext), *_ch(zeta=zeta)[:4], public_inputs=_pi(c))
        assert _values(got_evals) == evals and np.array_equal(got_r, GO.to_limbs(r))
        got_evals, proof = _open(circ, c, z, T, log_ext, zeta=zeta)
        assert _values(got_evals) == evals
        assert proof.compress() == TO.g1_scalar(oracle, SO.proof_scalar(stack[0], stack[1], stack[2], V, S))
    finally:
        circ.close()


# ---- the resident chain --------------------------------------------------------------------------------------------------------
def test_quotient_device_then_open_device_gives_the_bytes_of_the_host_form(engines):
    n, t, log_ext = 256, 3, 2
    N, stride = n << log_ext, n + 5
    e = engines.bench_srs(SRS)
    c, z, T, coefs = _case(n, t)
    _, evals, _ = _lin(n, t, log_ext)
    circ = _create(e, c, log_ext)
    bufs = []
    try:
        def up(a):
            a = np.ascontiguousarray(a)
            bufs.append(e.dev_alloc(a.nbytes))
            e.dev_upload(bufs[-1], a)
            return bufs[-1]
        d_w, d_z, d_pi = up(_limbs(c.wires, stride)), up(GO.to_limbs(z)), up(_pi(c))
        bufs.append(e.dev_alloc((N - n) * 32))
        d_t = bufs[-1]
        circ.quotient_device(d_w, d_z, *_ch()[:3], d_t, d_public_inputs=d_pi, stride=stride)
        dev_evals, dev_proof = circ.open_device(d_w, d_z, d_t, *_ch(), d_public_inputs=d_pi, stride=stride)
        host_evals, host_proof = _open(circ, c, z, T, log_ext)
        assert _values(dev_evals) == _values(host_evals) == evals
        assert np.array_equal(dev_proof.p1, host_proof.p1)
    finally:
        for b in bufs:
            e.dev_free(b)
        circ.close()


# ---- errors, and the context afterwards ----------------------------------------------------------------------------------------
def _refused(e, status, call, message=None):
    with pytest.raises(K.KzgError) as ei:
        call()
    assert ei.value.status == status, ei.value
    if message is not None:
        assert message in K.load_library().kzg_last_error(e._h)


def test_errors_leave_the_context_serving(engines, oracle):
    n, t, log_ext = 256, 3, 2
    e, small = engines.bench_srs(SRS), engines.bench_srs(64)
    c, z, T, coefs = _case(n, t)
    _, evals, stack = _lin(n, t, log_ext)
    want = TO.g1_scalar(oracle, SO.proof_scalar(stack[0], stack[1], stack[2], V, S))
    circ, on_small = _create(e, c, log_ext), _create(small, c, log_ext)
    try:
        def good():
            got_evals, proof = _open(circ, c, z, T, log_ext)
            assert _values(got_evals) == evals and proof.compress() == want
        good()
        bad = LO.chunks(T, n, log_ext)
        bad[1][n - 1] = (bad[1][n - 1] + 1) % R  # one coefficient of T
        _refused(e, K.KZG_ERR_REMAINDER, lambda: _open(circ, c, z, [v for ch in bad for v in ch], log_ext), b"does not vanish at zeta")
        good()
        wires = [list(col) for col in c.wires]  # one wire value: the evaluations are another polynomial's
        wires[0][3] = (wires[0][3] + 1) % R
        other = CO.Circuit(c.ks, wires, c.sigmas, c.q_lin, c.q_mul, c.q_const, c.pi)
        _refused(e, K.KZG_ERR_REMAINDER, lambda: _open(circ, other, z, T, log_ext), b"does not vanish at zeta")
        good()
        not_fr = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)

        class NotBelowR:
            def limbs(self):
                return not_fr
        for pos in range(5):  # every challenge in turn
            ch = _ch()
            ch[pos] = NotBelowR()
            _refused(e, K.KZG_ERR_INVALID_ARG, lambda: circ.open(_limbs(c.wires), GO.to_limbs(z), _t_limbs(T, n, log_ext), *ch,
                                                                public_inputs=_pi(c)))
        good()
        # a circuit of another context
        _refused(small, K.KZG_ERR_INVALID_ARG, lambda: circ.open(_limbs(c.wires), GO.to_limbs(z), _t_limbs(T, n, log_ext), *_ch(),
                                                                 public_inputs=_pi(c), engine=small), b"not a circuit alive on this context")
        # a setup shorter than n - 1: the linearisation needs none, the opening does
        _refused(small, K.KZG_ERR_DEGREE_TOO_HIGH, lambda: _open(on_small, c, z, T, log_ext))
        got_evals, got_r = on_small.linearise(_limbs(c.wires), GO.to_limbs(z), _t_limbs(T, n, log_ext), *_ch()[:4], public_inputs=_pi(c))
        assert _values(got_evals) == evals
        # a stride below n
        lib = K.load_library()
        a = np.ascontiguousarray(_limbs(c.wires))
        zz, tc, ev, p1 = GO.to_limbs(z), _t_limbs(T, n, log_ext), np.zeros((2 * t, 4), dtype=np.uint64), np.zeros(18, dtype=np.uint64)
        ptr = lambda x: x.ctypes.data_as(C.c_void_p)
        lim = [ptr(x.limbs()) for x in _ch()]
        assert lib.kzg_circuit_open(e._h, circ._c, ptr(a), n - 1, ptr(zz), None, ptr(tc), *lim, ptr(ev), ptr(p1)) == K.KZG_ERR_INVALID_ARG
        assert lib.kzg_circuit_open(e._h, circ._c, ptr(a), n, ptr(zz), None, None, *lim, ptr(ev), ptr(p1)) == K.KZG_ERR_INVALID_ARG
        assert not p1.any()  # out_p1 is left unwritten
        good()
    finally:
        circ.close()
        on_small.close()


def test_destroy_right_after_the_call_and_a_second_opening_with_other_challenges(engines, oracle):
    n, t, log_ext = 256, 3, 2
    e = engines.bench_srs(SRS)
    c, z, T, coefs = _case(n, t)
    zeta2, v2 = (ZETA * 3 + 1) % R, (V * 5 + 2) % R
    r2, evals2, stack2 = _lin(n, t, log_ext, True, zeta2)
    _, evals, stack = _lin(n, t, log_ext)
    circ = _create(e, c, log_ext)
    try:
        first = _open(circ, c, z, T, log_ext)
        # another shape in between: the workspaces grow and are reused
        cb, zb, Tb, _ = _case(64, 7)
        other = _create(e, cb, 3)
        got = _open(other, cb, zb, Tb, 3)
        other.close()  # right after the call
        assert _values(got[0]) == _lin(64, 7, 3)[1]
        second = _open(circ, c, z, T, log_ext, zeta=zeta2, v=v2)
        again = _open(circ, c, z, T, log_ext)
    finally:
        circ.close()
    assert _values(first[0]) == evals and _values(second[0]) == evals2
    assert first[1].compress() == again[1].compress() == TO.g1_scalar(oracle, SO.proof_scalar(stack[0], stack[1], stack[2], V, S))
    assert second[1].compress() == TO.g1_scalar(oracle, SO.proof_scalar(stack2[0], stack2[1], stack2[2], v2, S))


# ---- contexts without a setup, and over several devices -------------------------------------------------------------------------
def test_linearise_needs_no_setup_and_open_says_so(engines):
    n, t, log_ext = 256, 3, 2
    c, z, T, coefs = _case(n, t)
    r, evals, _ = _lin(n, t, log_ext)
    bare = K.Engine(0)  # no SRS was ever loaded: the slots' MSM workspaces do not exist
    try:
        circ = _create(bare, c, log_ext)
        got_evals, got_r = circ.linearise(_limbs(c.wires, n + 5), GO.to_limbs(z), _t_limbs(T, n, log_ext), *_ch()[:4], public_inputs=_pi(c))
        assert _values(got_evals) == evals and np.array_equal(got_r, GO.to_limbs(r))
        _refused(bare, K.KZG_ERR_NO_SRS, lambda: _open(circ, c, z, T, log_ext))
        got_evals, got_r = circ.linearise(_limbs(c.wires), GO.to_limbs(z), _t_limbs(T, n, log_ext), *_ch()[:4], public_inputs=_pi(c))
        assert _values(got_evals) == evals and np.array_equal(got_r, GO.to_limbs(r))
    finally:
        bare.close()  # frees the circuit still alive on it


def test_multi_device_contexts_follow_the_quotient(engines, oracle):
    n, t, log_ext = 256, 3, 2
    c, z, T, coefs = _case(n, t)
    r, evals, stack = _lin(n, t, log_ext)
    want = TO.g1_scalar(oracle, SO.proof_scalar(stack[0], stack[1], stack[2], V, S))
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(BT.BENCH_SECRET_BE, n)
        circ = _create(rep, c, log_ext)
        got_evals, proof = _open(circ, c, z, T, log_ext)  # forwarded to the circuit's device
        assert _values(got_evals) == evals and proof.compress() == want
        got_evals, got_r = circ.linearise(_limbs(c.wires), GO.to_limbs(z), _t_limbs(T, n, log_ext), *_ch()[:4], public_inputs=_pi(c))
        assert _values(got_evals) == evals and np.array_equal(got_r, GO.to_limbs(r))
        _refused(rep, K.KZG_ERR_INVALID_ARG, lambda: circ.open_device(1 << 20, 2 << 20, 3 << 20, *_ch()))  # single-device only
        circ.close()
    finally:
        rep.close()
    split = K.Engine(devices=[0, 0])
    try:
        split.srs_generate(BT.BENCH_SECRET_BE, n)
        circ = _create(split, c, log_ext)
        with pytest.raises(K.KzgError) as ei:
            _open(circ, c, z, T, log_ext)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG and "range-split" in str(ei.value)
        got_evals, got_r = circ.linearise(_limbs(c.wires), GO.to_limbs(z), _t_limbs(T, n, log_ext), *_ch()[:4], public_inputs=_pi(c))
        assert _values(got_evals) == evals and np.array_equal(got_r, GO.to_limbs(r))
        circ.close()
    finally:
        split.close()
