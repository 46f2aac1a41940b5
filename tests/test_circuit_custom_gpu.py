"""GPU: circuit proofs with custom gates -- kzg_circuit_create_custom, kzg_circuit_custom_gate (the test
hook of k_cg_gate), kzg_circuit_custom_quotient plain and blinded, the selector columns through kzg_circuit_column_device, and the
proof in one call, kzg_circuit_custom_prove / _device, plain and blinded.

Everything is compared limb for limb or byte for byte with tests/circuit_custom_oracle.py; the plain T also bit for bit with
kzg_circuit_quotient given the oracle's G' on the coset; every proof is verified by kzg_circuit_custom_verify_proof.  The cases
are tests/circuit_custom_cases.py's, each built once; there are no tolerances."""
import ctypes as C

import numpy as np
import pytest

import bigint_twin as BT
import blind_oracle as BO
import circuit_custom_cases as CC
import circuit_custom_oracle as CX
import circuit_oracle as CO
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import perm_quotient_oracle as PQ
import transcript_oracle as TR

pytestmark = pytest.mark.gpu
R = CX.R
SRS = 4096 + 16  # a blinded proof at n = 4096 commits to n + t + 3 coefficients
BE, GA, AL = (K.Scalar(v) for v in (CC.BETA, CC.GAMMA, CC.ALPHA))
S = BT.fr_from_be_bytes(BT.BENCH_SECRET_BE)
FILL = 0x5A
ids = lambda s: "n%d_t%d_e%d_%s" % (s[0], s[1], 1 << s[2], "_".join("".join(map(str, r)) for r in s[3]))


def _limbs(cols, stride=None):
    """columns -> (t, stride, 4); the rows past n hold values that are not the columns'"""
    n = len(cols[0])
    stride = n if stride is None else stride
    out = np.empty((len(cols), stride, 4), dtype=np.uint64)
    for j, c in enumerate(cols):
        out[j] = GO.to_limbs(list(c) + [0xBAD + i for i in range(stride - n)])
    return out


def _create(e, cc, log_ext, stride=None, want_key=False, exps=None):
    c = cc.circuit
    return e.circuit_create_custom(_limbs(c.q_lin, stride), GO.to_limbs(c.q_mul), GO.to_limbs(c.q_const), _limbs(c.sigmas, stride),
                                   [K.Scalar(k) for k in c.ks], log_ext, _limbs(cc.q_custom, stride), cc.exps if exps is None else exps,
                                   n=c.n, want_key=want_key)


def _plain(e, c, log_ext, want_key=False):
    return e.circuit_create(_limbs(c.q_lin), GO.to_limbs(c.q_mul), GO.to_limbs(c.q_const), _limbs(c.sigmas), [K.Scalar(k) for k in c.ks],
                            log_ext, want_key=want_key)


def _pi(c):
    return None if c.pi is None else GO.to_limbs(c.pi)


def _invalid(call):
    with pytest.raises(K.KzgError) as ei:
        call()
    assert ei.value.status == K.KZG_ERR_INVALID_ARG, ei.value
    return ei.value


# ---- the kernel and the quotient, limb for limb, at every shape ------------------------------------------------------------------
@pytest.mark.parametrize("shape", CC.SHAPES, ids=ids)
def test_gate_and_quotient_against_the_oracle(engines, shape):
    n, t, log_ext, exps = shape
    e = engines.bench_srs(SRS)
    cs = CC.case(n, t, log_ext, exps)
    c = cs.cc.circuit
    N = n << log_ext
    circ = _create(e, cs.cc, log_ext, stride=n + 3)
    try:
        wires = _limbs(c.wires, n + 5)
        ext = PQ.coset_extend(cs.gprime or [0], NO.log2_exact(n) + log_ext)  # the oracle's G' on the coset
        assert np.array_equal(circ.custom_gate(wires, n=n), GO.to_limbs(ext))
        coeffs, points = circ.custom_quotient(wires, GO.to_limbs(cs.z), AL, BE, GA, public_inputs=_pi(c), n=n)
        full = cs.quotient[:N - n]
        assert not any(cs.quotient[N - n:]) and np.array_equal(coeffs, GO.to_limbs(full))
        assert len(points) == (1 << log_ext) - 1
        for k, point in enumerate(points):
            assert np.array_equal(point.p1, e.commit_limbs(GO.to_limbs(full[k * n:(k + 1) * n])).p1), k
        # bit for bit what kzg_circuit_quotient returns given the oracle's G' on the coset (the handle's custom terms are ignored)
        old_c, old_p = circ.quotient(wires, GO.to_limbs(cs.z), AL, BE, GA, public_inputs=_pi(c), gate=GO.to_limbs(ext), n=n)
        assert np.array_equal(coeffs, old_c)
        assert all(np.array_equal(x.p1, y.p1) for x, y in zip(points, old_p))
        if CC.blinded_legal(*shape):
            bl, _, Tb = cs.blinded()
            arr = GO.to_limbs(bl.flat())
            cb, pb = circ.custom_quotient(wires, GO.to_limbs(cs.z), AL, BE, GA, blinders=arr, public_inputs=_pi(c), n=n)
            assert np.array_equal(cb, GO.to_limbs(Tb))
            for k, ch in enumerate(BO.chunks(Tb, n, t, log_ext, bl)):
                assert np.array_equal(pb[k].p1, e.commit_limbs(GO.to_limbs(ch)).p1), k
        else:
            arr = GO.to_limbs(cs.blinders().flat())
            err = _invalid(lambda: circ.custom_quotient(wires, GO.to_limbs(cs.z), AL, BE, GA, blinders=arr, public_inputs=_pi(c), n=n))
            assert "blinded quotient" in str(err)
    finally:
        circ.close()


# ---- the key: commitments and the resident selector columns ---------------------------------------------------------------------
def test_key_commitments_and_resident_custom_columns(engines):
    n, t, log_ext, exps = CC.SHAPES[4]  # n = 256
    g, N = len(exps), n << log_ext
    e = engines.bench_srs(SRS)
    cs = CC.case(n, t, log_ext, exps)
    sbox = CC.case(*CC.SBOX)
    circ = _create(e, cs.cc, log_ext, stride=n + 3, want_key=True)
    two = _create(e, sbox.cc, CC.SBOX[2], want_key=True)
    plain = _plain(e, cs.cc.circuit, log_ext, want_key=True)
    try:
        cols = cs.cc.key_columns()
        assert len(circ.key) == 2 * t + 2 + g and circ.g == g and len(two.key) == 2 * 3 + 2 + 2
        for j, col in enumerate(cols):  # kzg_circuit_create's order, then qx_0..
            assert np.array_equal(circ.key[j].p1, e.commit_evaluations_limbs(GO.to_limbs(col)).p1), j
        for j, col in enumerate(sbox.cc.key_columns()):
            assert np.array_equal(two.key[j].p1, e.commit_evaluations_limbs(GO.to_limbs(col)).p1), j
        for j in range(2 * t + 2):
            assert np.array_equal(circ.key[j].p1, plain.key[j].p1), j
        ext = e.coset_extend_limbs(_limbs(cols[2 * t + 2:]), NO.log2_exact(N))
        lib = K.load_library()

        def down(p, rows):
            got = np.zeros((rows, 4), dtype=np.uint64)
            assert lib.kzg_dev_download(e._h, got.ctypes.data, C.c_void_p(p), rows * 32) == 0
            return got
        for s in range(g):
            col, w = cols[2 * t + 2 + s], K.KZG_CIRCUIT_COL_CUSTOM + s
            p, ln = circ.column_device(w, K.KZG_CIRCUIT_VALUES)
            assert ln == n and np.array_equal(down(p, n), GO.to_limbs(col)), s
            p, ln = circ.column_device(w, K.KZG_CIRCUIT_COEFFS)
            assert ln == n and np.array_equal(down(p, n), GO.to_limbs(NO.intt(col))), s
            p, ln = circ.column_device(w, K.KZG_CIRCUIT_COSET)
            assert ln == N and np.array_equal(down(p, N), ext[s]), s
        p0, _ = circ.column_device(K.KZG_CIRCUIT_COL_QLIN, K.KZG_CIRCUIT_COEFFS)
        px, _ = circ.column_device(K.KZG_CIRCUIT_COL_CUSTOM, K.KZG_CIRCUIT_COEFFS)
        assert px == p0 + (2 * t + 2) * n * 32  # behind the sigmas, contiguous
        for circuit, w in ((circ, K.KZG_CIRCUIT_COL_CUSTOM + g), (plain, K.KZG_CIRCUIT_COL_CUSTOM), (circ, K.KZG_CIRCUIT_COL_TABLE),
                           (circ, K.KZG_CIRCUIT_COL_QLOOKUP)):
            _invalid(lambda: circuit.column_device(w, K.KZG_CIRCUIT_VALUES))
        # a circuit without custom gates has no custom gate, quotient or proof
        wires = _limbs(cs.cc.circuit.wires)
        for call in (lambda: plain.custom_gate(wires), lambda: plain.custom_quotient(wires, GO.to_limbs(cs.z), AL, BE, GA),
                     lambda: plain.custom_prove(wires, _pi(cs.cc.circuit))):
            assert "without custom gates" in str(_invalid(call))
    finally:
        for x in (circ, two, plain):
            x.close()


def test_shape_rules_of_create(engines):
    n, t, log_ext, exps = CC.SBOX
    e = engines.bench_srs(SRS)
    cc = CC.case(*CC.SBOX).cc
    _create(e, cc, log_ext).close()
    for bad in ([[5, 0, 0], [0, 0, 0]], [[8, 0, 0], [0, 2, 1]], [[5, 2, 1], [0, 2, 1]]):  # a term of degree 0; an exponent above 7; d_max = 8 > e - 1
        _invalid(lambda: _create(e, cc, log_ext, exps=bad))
    _invalid(lambda: _create(e, cc, 2))  # e = 4 < d_max + 1 = 6
    wide = CC.case(*CC.WIDE).cc
    four = CX.CustomCircuit(wide.circuit, wide.q_custom + wide.q_custom[:1], wide.exps + wide.exps[:1])
    _invalid(lambda: _create(e, four, CC.WIDE[2]))  # 33 columns at zeta
    nine = CX.CustomCircuit(cc.circuit, [cc.q_custom[0]] * 9, [cc.exps[0]] * 9)
    _invalid(lambda: _create(e, nine, log_ext))  # g = 9
    lib, h = K.load_library(), C.c_void_p()
    a = _limbs(cc.circuit.q_lin)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    ex = np.array(cc.exps, dtype=np.uint8)
    for q, x, stride in ((None, ptr(ex), n), (ptr(a), None, n), (ptr(a), ptr(ex), n - 1)):
        rc = lib.kzg_circuit_create_custom(e._h, ptr(a), ptr(a), ptr(a), ptr(a), n, t, n, ptr(a), log_ext, q, 2, stride, x, None, C.byref(h))
        assert rc == K.KZG_ERR_INVALID_ARG and not h.value


# ---- the proof in one call -------------------------------------------------------------------------------------------------------
def _proof(oracle, shape, blinded=False, with_pi=True, n_public=None):
    """tests/circuit_custom_oracle.py's proof under the bench secret, computed once"""
    n, t, log_ext, exps = shape

    def make():
        cs = CC.case(n, t, log_ext, exps, with_pi)
        return CX.prove(oracle, cs.cc, log_ext, cs.blinders() if blinded else cs.zero, S, n_public)
    return CC.memo(("bench proof", shape, blinded, with_pi, n_public), make)


def _setup(oracle):
    """[s^0]G1 and [s^j]G2, j <= 2, of the bench secret"""
    return CC.memo("setup", lambda: (np.stack([oracle.p1_generator()]), np.stack([K.srs_g2_at(BT.BENCH_SECRET_BE, j) for j in range(3)])))


def _pub(d):
    return GO.to_limbs(d["public"]) if d["public"] else None


def _bl(shape, d=None):
    cs = CC.case(*shape)
    return GO.to_limbs(cs.blinders().flat())


def _raw(e, circ, wires, pub, blinders=None, fn="kzg_circuit_custom_prove", stride=None):
    """the C call on a pre-filled output: (status, the output bytes)"""
    rows = np.ascontiguousarray(np.stack([p.p1 for p in circ.key]), dtype=np.uint64)
    out = np.full(K.circuit_proof_size(circ.t, circ.log_ext), FILL, dtype=np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    w = np.ascontiguousarray(wires)
    rc = getattr(e._lib, fn)(e._h, circ._c, ptr(rows), ptr(w), w.shape[1] if stride is None else stride, ptr(pub),
                             0 if pub is None else pub.shape[0], ptr(blinders), ptr(out))
    return rc, out


@pytest.mark.parametrize("with_pi", [True, False], ids=["pi", "no_pi"])
@pytest.mark.parametrize("shape", CC.SHAPES, ids=ids)
def test_proof_bytes_against_the_oracle_and_verified(engines, oracle, shape, with_pi):
    n, t, log_ext, exps = shape
    e = engines.bench_srs(SRS)
    d = _proof(oracle, shape, with_pi=with_pi)
    cc = d["cc"]
    circ = _create(e, cc, log_ext, want_key=True)
    try:
        assert [k.compress() for k in circ.key] == d["key48"]
        g1, g2 = _setup(oracle)
        shifts, public = [K.Scalar(k) for k in cc.circuit.ks], [K.Scalar(p) for p in d["public"]]
        proof = circ.custom_prove(_limbs(cc.circuit.wires, n + 5), _pub(d), n=n)  # wire stride n + 5
        want = d["proof"]
        assert proof == want, [name for name, f in TR.split(proof, t, log_ext).items() if f != TR.split(want, t, log_ext)[name]]
        assert K.circuit_custom_verify_proof(circ.key, n, log_ext, cc.exps, shifts, public, proof, g1, g2)
        got = K.circuit_custom_proof_challenges(circ.key, n, log_ext, cc.exps, shifts, public, proof)
        assert tuple(x.v for x in got) == tuple(d[k] for k in ("beta", "gamma", "alpha", "zeta", "v"))
        assert circ.custom_prove(_limbs(cc.circuit.wires), _pub(d)) == want  # packed wires, a second call
        if CC.blinded_legal(*shape):
            db = _proof(oracle, shape, blinded=True, with_pi=with_pi)
            arr = GO.to_limbs(CC.case(n, t, log_ext, exps, with_pi).blinders().flat())
            got = circ.custom_prove(_limbs(cc.circuit.wires, n + 5), _pub(db), arr, n=n)
            assert got == db["proof"], [name for name, f in TR.split(got, t, log_ext).items() if f != TR.split(db["proof"], t, log_ext)[name]]
            assert got != want and K.circuit_custom_verify_proof(circ.key, n, log_ext, cc.exps, shifts, public, got, g1, g2)
            # all blinders zero: the plain proof
            assert circ.custom_prove(_limbs(cc.circuit.wires), _pub(d), np.zeros_like(arr)) == want
    finally:
        circ.close()


def test_partial_public_inputs(engines, oracle):
    """n_public < n: the later rows of PI are zero in the statement and on the device"""
    n, t, log_ext, exps = CC.SBOX
    e = engines.bench_srs(SRS)
    cs = CC.case(*CC.SBOX)
    assert cs.cc.circuit.pi[n - 1] == 0  # (rows i % 3 != 0 hold no public input)
    d = _proof(oracle, CC.SBOX, n_public=n - 1)
    assert len(d["public"]) == n - 1 and d["proof"] != _proof(oracle, CC.SBOX)["proof"]
    circ = _create(e, cs.cc, log_ext, want_key=True)
    try:
        proof = circ.custom_prove(_limbs(cs.cc.circuit.wires), _pub(d))
        assert proof == d["proof"]
        g1, g2 = _setup(oracle)
        assert K.circuit_custom_verify_proof(circ.key, n, log_ext, cs.cc.exps, [K.Scalar(k) for k in cs.cc.circuit.ks],
                                             [K.Scalar(p) for p in d["public"]], proof, g1, g2)
    finally:
        circ.close()


def test_kzg_circuit_prove_on_a_custom_handle_gives_the_base_statements_status(engines, oracle):
    n, t, log_ext, exps = CC.SBOX
    e = engines.bench_srs(SRS)
    d = _proof(oracle, CC.SBOX)
    cc = d["cc"]
    c = cc.circuit
    # the base gate does not hold on these wires: the plain prover's quotient leaves a remainder
    circ = _create(e, cc, log_ext, want_key=True)
    # ... and with q_C put back so that the base gate holds, the plain proof is that of the base circuit, the custom terms ignored
    base = CO.Circuit(c.ks, c.wires, c.sigmas, c.q_lin, c.q_mul, [0] * n, c.pi)
    base.q_const = [(-v) % R for v in CO.gate_rows(base)]
    held = _create(e, CX.CustomCircuit(base, cc.q_custom, cc.exps), log_ext, want_key=True)
    try:
        wires, pub = _limbs(c.wires), _pub(d)
        rc, out = _raw(e, circ, wires, pub, fn="kzg_circuit_prove")
        assert rc == K.KZG_ERR_REMAINDER and (out == FILL).all() and b"not divisible" in e._lib.kzg_last_error(e._h)
        plain = CC.memo("base plain proof", lambda: TR.prove(oracle, base, log_ext, BO.Blinders.zero(t, log_ext), S))
        rc, out = _raw(e, held, wires, pub, fn="kzg_circuit_prove")
        assert rc == 0 and out.tobytes() == plain["proof"]
        rc, out = _raw(e, held, wires, pub)  # the custom statement does not hold there
        assert rc == K.KZG_ERR_REMAINDER and (out == FILL).all()
        assert circ.custom_prove(wires, pub) == d["proof"]
    finally:
        circ.close()
        held.close()


def test_prover_statuses_leave_the_output_untouched_and_the_context_serving(engines, oracle):
    n, t, log_ext, exps = CC.REFUSED_BLINDED
    e = engines.bench_srs(SRS)
    d = _proof(oracle, CC.REFUSED_BLINDED)
    cc = d["cc"]
    c = cc.circuit
    wires, pub = _limbs(c.wires, n + 5), _pub(d)
    circ = _create(e, cc, log_ext, want_key=True)
    plain = _plain(e, c, log_ext)
    plain.key = circ.key
    try:
        def good():
            rc, out = _raw(e, circ, wires, pub)
            assert rc == 0 and out.tobytes() == d["proof"]

        def refused(status, message, *args, **kw):
            rc, out = _raw(e, *args, **kw)
            assert rc == status and (out == FILL).all(), (rc, message)
            if message:
                assert message in e._lib.kzg_last_error(e._h), e._lib.kzg_last_error(e._h)
            good()

        good()
        # the blinded refusal: 7 n + 7 > L_T
        arr = GO.to_limbs(CC.case(*CC.REFUSED_BLINDED).blinders().flat())
        refused(K.KZG_ERR_INVALID_ARG, b"blinded quotient of custom gates", circ, wires, pub, arr)
        # an unsatisfied custom gate row
        row = next(i for i in range(n) if cc.q_custom[0][i])
        moved = wires.copy()
        moved_val = (c.wires[0][row] + 1) % R
        moved[0, row] = GO.to_limbs([moved_val])[0]
        # (the permutation breaks first when a copied wire moves: move the selector instead -- another key, the same wires)
        qx = [list(col) for col in cc.q_custom]
        qx[0][row] = (qx[0][row] + 1) % R
        broken = _create(e, CX.CustomCircuit(c, qx, cc.exps), log_ext, want_key=True)
        try:
            refused(K.KZG_ERR_REMAINDER, b"not divisible", broken, wires, pub)
        finally:
            broken.close()
        refused(K.KZG_ERR_REMAINDER, None, circ, moved, pub)
        # argument errors
        not_fr = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
        refused(K.KZG_ERR_INVALID_ARG, b"without custom gates", plain, wires, pub)
        refused(K.KZG_ERR_INVALID_ARG, None, circ, wires, pub, stride=n - 1)
        refused(K.KZG_ERR_INVALID_ARG, None, circ, wires, np.concatenate([pub, pub[:1]]))  # n_public = n + 1
        bad_pub = pub.copy()
        bad_pub[n - 1] = not_fr
        refused(K.KZG_ERR_INVALID_ARG, b"public input is not below r", circ, wires, bad_pub)
        other = engines.bench_srs(n)
        rc, out = _raw(other, circ, wires, pub)  # a circuit of another context
        assert rc == K.KZG_ERR_INVALID_ARG and (out == FILL).all()
        good()
        short = engines.bench_srs(n // 2)  # fewer than n points
        nokey = _create(short, cc, log_ext)
        nokey.key = circ.key
        rc, out = _raw(short, nokey, wires, pub)
        assert rc == K.KZG_ERR_DEGREE_TOO_HIGH and (out == FILL).all()
        nokey.close()
    finally:
        circ.close()
        plain.close()


@pytest.mark.parametrize("shape", [CC.SBOX, CC.SHAPES[4], CC.SHAPES[1]], ids=ids)
def test_device_form_inside_guard_bands(engines, oracle, shape):
    import device_arena as DA
    n, t, log_ext, exps = shape
    e = engines.bench_srs(SRS)
    d = _proof(oracle, shape)
    cc = d["cc"]
    circ = _create(e, cc, log_ext, want_key=True)
    try:
        with DA.Arena(e, seed=n + t) as arena:
            r_w = arena.region(n, t, n + 5, "wires", data=_limbs(cc.circuit.wires, n))
            arena.upload()
            proof = circ.custom_prove_device(r_w.ptr, _pub(d), stride=n + 5)
            blinded = None
            if CC.blinded_legal(*shape):
                blinded = circ.custom_prove_device(r_w.ptr, _pub(d), _bl(shape), stride=n + 5)
            arena.check_untouched()
        assert proof == d["proof"]
        if blinded is not None:
            assert blinded == _proof(oracle, shape, blinded=True)["proof"]
    finally:
        circ.close()


def test_after_a_larger_plain_proof_on_the_same_context(oracle):
    """workspaces and cross-round buffers grown by one call are reused or regrown by the next: a custom proof at 8 rows, a plain
    proof at 2048 rows, the custom proofs again"""
    e = K.SetupArtifactsGenerator(BT.BENCH_SECRET_BE).take(2048 + 16)
    try:
        d, db = _proof(oracle, CC.SBOX), _proof(oracle, CC.SBOX, blinded=True)
        cc = d["cc"]
        circ = _create(e, cc, CC.SBOX[2], want_key=True)
        wires, pub = _limbs(cc.circuit.wires, 8 + 5), _pub(d)
        assert circ.custom_prove(wires, pub, n=8) == d["proof"]
        big_shape = CC.SHAPES[5]
        big_cc = CC.case(*big_shape).cc
        bc = big_cc.circuit
        base = CO.Circuit(bc.ks, bc.wires, bc.sigmas, bc.q_lin, bc.q_mul, [0] * bc.n, bc.pi)
        base.q_const = [(-v) % R for v in CO.gate_rows(base)]
        big_plain = CC.memo("big plain proof", lambda: TR.prove(oracle, base, 2, BO.Blinders.zero(3, 2), S))
        big = _plain(e, base, 2, want_key=True)
        assert big.prove(_limbs(base.wires), GO.to_limbs(big_plain["public"]), None) == big_plain["proof"]
        assert circ.custom_prove(wires, pub, n=8) == d["proof"]
        assert circ.custom_prove(wires, pub, _bl(CC.SBOX), n=8) == db["proof"]
        bigx = _create(e, big_cc, 2, want_key=True)
        assert bigx.custom_prove(_limbs(bc.wires), GO.to_limbs(big_plain["public"])) == _proof(oracle, big_shape)["proof"]
        assert circ.custom_prove(wires, pub, n=8) == d["proof"]
        for x in (big, bigx, circ):
            x.close()
    finally:
        e.close()


def test_on_two_device_contexts(oracle):
    n, t, log_ext, exps = CC.SBOX
    d, db = _proof(oracle, CC.SBOX), _proof(oracle, CC.SBOX, blinded=True)
    cs = CC.case(*CC.SBOX)
    cc = d["cc"]
    wires, pub = _limbs(cc.circuit.wires), _pub(d)
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(BT.BENCH_SECRET_BE, n + t + 3)
        circ = _create(rep, cc, log_ext, want_key=True)
        assert len(circ.key) == 2 * t + 2 + len(exps)
        ext = PQ.coset_extend(cs.gprime, NO.log2_exact(n) + log_ext)
        assert np.array_equal(circ.custom_gate(wires), GO.to_limbs(ext))
        coeffs, _ = circ.custom_quotient(wires, GO.to_limbs(cs.z), AL, BE, GA, public_inputs=_pi(cc.circuit))
        assert np.array_equal(coeffs, GO.to_limbs(cs.quotient[:(n << log_ext) - n]))
        assert circ.custom_prove(wires, pub) == d["proof"]  # forwarded to the circuit's device
        assert circ.custom_prove(wires, pub, _bl(CC.SBOX)) == db["proof"]
        with pytest.raises(K.KzgError) as ei:
            circ.custom_prove_device(1 << 20, pub)  # single-device only
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        circ.close()
    finally:
        rep.close()
    split = K.Engine(devices=[0, 0])
    try:
        split.srs_generate(BT.BENCH_SECRET_BE, n)
        circ = _create(split, cc, log_ext)
        circ.key = [K.G1Point(oracle.p1_mult(oracle.p1_generator(), s % R)) for s in d["key_s"]]
        with pytest.raises(K.KzgError) as ei:
            circ.custom_prove(wires, pub)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG and "range-split" in str(ei.value)
        circ.close()
    finally:
        split.close()
