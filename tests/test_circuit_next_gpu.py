"""GPU: circuit proofs whose custom gates read the next row -- kzg_circuit_create_custom_next,
kzg_circuit_custom_next_gate (the test hook of k_cgn_gate), kzg_circuit_custom_next_quotient and the proof in one call,
kzg_circuit_custom_next_prove / _device.

Everything is compared limb for limb or byte for byte with tests/circuit_next_oracle.py; T also bit for bit with
kzg_circuit_quotient given the oracle's G' on the coset; the proof element with kzg_open_sets of the oracle's stack on the three
sets; every proof is verified by kzg_circuit_custom_next_verify_proof.  The cases are tests/circuit_next_cases.py's, each built
once; there are no tolerances."""
import ctypes as C

import numpy as np
import pytest

import bigint_twin as BT
import blind_oracle as BO
import circuit_custom_oracle as CX
import circuit_next_cases as NC
import circuit_next_oracle as CN
import circuit_oracle as CO
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import perm_quotient_oracle as PQ
import transcript_oracle as TR

pytestmark = pytest.mark.gpu
R = CN.R
SRS = 4096 + 16
BE, GA, AL = (K.Scalar(v) for v in (NC.BETA, NC.GAMMA, NC.ALPHA))
S = BT.fr_from_be_bytes(BT.BENCH_SECRET_BE)
FILL = 0x5A
_rows = lambda m: "_".join("".join(map(str, r)) for r in m)
ids = lambda s: "n%d_t%d_e%d_%s_next_%s" % (s[0], s[1], 1 << s[2], _rows(s[3]), _rows(s[4]))


def _limbs(cols, stride=None):
    """columns -> (t, stride, 4); the rows past n hold values that are not the columns'"""
    n = len(cols[0])
    stride = n if stride is None else stride
    out = np.empty((len(cols), stride, 4), dtype=np.uint64)
    for j, c in enumerate(cols):
        out[j] = GO.to_limbs(list(c) + [0xBAD + i for i in range(stride - n)])
    return out


def _create(e, nc, log_ext, stride=None, want_key=False, exps=None, exps_next=None, custom_only=False):
    c = nc.circuit
    args = (_limbs(c.q_lin, stride), GO.to_limbs(c.q_mul), GO.to_limbs(c.q_const), _limbs(c.sigmas, stride), [K.Scalar(k) for k in c.ks],
            log_ext, _limbs(nc.q_custom, stride), nc.exps if exps is None else exps)
    if custom_only:
        return e.circuit_create_custom(*args, n=c.n, want_key=want_key)
    return e.circuit_create_custom_next(*args, nc.exps_next if exps_next is None else exps_next, n=c.n, want_key=want_key)


def _pi(c):
    return None if c.pi is None else GO.to_limbs(c.pi)


def _invalid(call):
    with pytest.raises(K.KzgError) as ei:
        call()
    assert ei.value.status == K.KZG_ERR_INVALID_ARG, ei.value
    return ei.value


# ---- the kernel and the quotient, limb for limb, at every shape ------------------------------------------------------------------
@pytest.mark.parametrize("shape", NC.SHAPES, ids=ids)
def test_gate_and_quotient_against_the_oracle(engines, shape):
    n, t, log_ext, exps, exps_next = shape
    e = engines.bench_srs(SRS)
    cs = NC.case(n, t, log_ext, exps, exps_next)
    c = cs.nc.circuit
    N = n << log_ext
    circ = _create(e, cs.nc, log_ext, stride=n + 3)
    try:
        wires = _limbs(c.wires, n + 5)
        ext = PQ.coset_extend(cs.gprime or [0], NO.log2_exact(n) + log_ext)  # the oracle's G' on the coset
        assert np.array_equal(circ.custom_next_gate(wires, n=n), GO.to_limbs(ext))
        coeffs, points = circ.custom_next_quotient(wires, GO.to_limbs(cs.z), AL, BE, GA, public_inputs=_pi(c), n=n)
        full = cs.quotient[:N - n]
        assert not any(cs.quotient[N - n:]) and np.array_equal(coeffs, GO.to_limbs(full))
        assert len(points) == (1 << log_ext) - 1
        for k, point in enumerate(points):
            assert np.array_equal(point.p1, e.commit_limbs(GO.to_limbs(full[k * n:(k + 1) * n])).p1), k
        # bit for bit what kzg_circuit_quotient returns given the oracle's G' on the coset (the handle's custom terms are ignored)
        old_c, old_p = circ.quotient(wires, GO.to_limbs(cs.z), AL, BE, GA, public_inputs=_pi(c), gate=GO.to_limbs(ext), n=n)
        assert np.array_equal(coeffs, old_c)
        assert all(np.array_equal(x.p1, y.p1) for x, y in zip(points, old_p))
    finally:
        circ.close()


def test_key_commitments_and_the_two_kinds_of_handle(engines):
    n, t, log_ext, exps, exps_next = NC.BOTH_ROWS
    g = len(exps)
    e = engines.bench_srs(SRS)
    cs = NC.case(*NC.BOTH_ROWS)
    circ = _create(e, cs.nc, log_ext, stride=n + 3, want_key=True)
    custom = _create(e, cs.nc, log_ext, want_key=True, custom_only=True)  # the same columns and p, no p'
    try:
        assert len(circ.key) == 2 * t + 2 + g and circ.g == g and circ.rho == 1 and custom.rho == 0
        for j, col in enumerate(cs.nc.key_columns()):  # kzg_circuit_create's order, then qx_0..
            assert np.array_equal(circ.key[j].p1, e.commit_evaluations_limbs(GO.to_limbs(col)).p1), j
            assert np.array_equal(circ.key[j].p1, custom.key[j].p1), j
        wires, z = _limbs(cs.nc.circuit.wires), GO.to_limbs(cs.z)
        # a kzg_circuit_custom_* call on a next-row handle would ignore p'
        for call in (lambda: circ.custom_gate(wires), lambda: circ.custom_quotient(wires, z, AL, BE, GA),
                     lambda: circ.custom_prove(wires, _pi(cs.nc.circuit)), lambda: circ.custom_prove_device(1 << 20, _pi(cs.nc.circuit))):
            assert "next-row terms" in str(_invalid(call))
        # ... and a custom handle has no p' for the new calls
        custom.rho = 1  # (the wrapper sizes the output by it)
        for call in (lambda: custom.custom_next_gate(wires), lambda: custom.custom_next_quotient(wires, z, AL, BE, GA),
                     lambda: custom.custom_next_prove(wires, _pi(cs.nc.circuit)),
                     lambda: custom.custom_next_prove_device(1 << 20, _pi(cs.nc.circuit))):
            assert "without next-row terms" in str(_invalid(call))
    finally:
        circ.close()
        custom.close()


def test_shape_rules_of_create(engines):
    n, t, log_ext, exps, exps_next = NC.NEXT_ONLY
    e = engines.bench_srs(SRS)
    nc = NC.case(*NC.NEXT_ONLY).nc
    _create(e, nc, log_ext).close()
    # rho = 0 (and a term of degree 0); an exponent above 7 in p'; d_max = 4 > e - 1; a term of degree 0
    for bad in ([[0, 0, 0], [0, 0, 0]], [[0, 1, 0], [0, 0, 8]], [[0, 1, 0], [0, 2, 2]], [[0, 1, 0], [0, 0, 0]]):
        _invalid(lambda: _create(e, nc, log_ext, exps_next=bad))
    _invalid(lambda: _create(e, nc, log_ext, exps=[[1, 0, 0], [1, 0, 0]], exps_next=[[0, 0, 0], [0, 0, 0]]))  # rho = 0 alone
    _invalid(lambda: _create(e, nc, log_ext, exps=[[8, 0, 0], [0, 0, 0]]))
    one = NC.case(2, 2, 2, ((1, 0),), ((0, 1),)).nc
    c1 = CO.satisfied(0, 2, 5, True)  # n = 1: w = 1
    _invalid(lambda: _create(e, CN.NextCircuit(c1, [[1]], one.exps, one.exps_next), 2))
    wide = NC.case(*NC.WIDE).nc
    four = CN.NextCircuit(wide.circuit, wide.q_custom + wide.q_custom[:1], wide.exps + wide.exps[:1], wide.exps_next + wide.exps_next[:1])
    _invalid(lambda: _create(e, four, NC.WIDE[2]))  # 33 columns at zeta
    lib, h = K.load_library(), C.c_void_p()
    a = _limbs(nc.circuit.q_lin)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    ex, en = np.array(nc.exps, dtype=np.uint8), np.array(nc.exps_next, dtype=np.uint8)
    for q, x, xn, stride in ((None, ptr(ex), ptr(en), n), (ptr(a), None, ptr(en), n), (ptr(a), ptr(ex), None, n), (ptr(a), ptr(ex), ptr(en), n - 1)):
        rc = lib.kzg_circuit_create_custom_next(e._h, ptr(a), ptr(a), ptr(a), ptr(a), n, t, n, ptr(a), log_ext, q, 2, stride, x, xn, None,
                                                C.byref(h))
        assert rc == K.KZG_ERR_INVALID_ARG and not h.value


# ---- the proof in one call -------------------------------------------------------------------------------------------------------
def _proof(oracle, shape, with_pi=True):
    """tests/circuit_next_oracle.py's proof under the bench secret, computed once"""
    n, t, log_ext, exps, exps_next = shape

    def make():
        cs = NC.case(n, t, log_ext, exps, exps_next, with_pi)
        return CN.prove(oracle, cs.nc, log_ext, S)
    return NC.memo(("bench proof", shape, with_pi), make)


def _setup(oracle):
    """[s^j]G1, j < 2, and [s^j]G2, j <= 2, of the bench secret"""
    return NC.memo("setup", lambda: (np.stack([oracle.p1_mult(oracle.p1_generator(), pow(S, j, R)) for j in range(2)]),
                                     np.stack([K.srs_g2_at(BT.BENCH_SECRET_BE, j) for j in range(3)])))


def _pub(d):
    return GO.to_limbs(d["public"]) if d["public"] else None


def _raw(e, circ, wires, pub, blinders=None, fn="kzg_circuit_custom_next_prove", stride=None, size=None):
    """the C call on a pre-filled output: (status, the output bytes)"""
    rows = np.ascontiguousarray(np.stack([p.p1 for p in circ.key]), dtype=np.uint64)
    out = np.full(K.circuit_custom_next_proof_size(circ.t, circ.log_ext, max(circ.rho, 1)) if size is None else size, FILL, dtype=np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    w = np.ascontiguousarray(wires)
    rc = getattr(e._lib, fn)(e._h, circ._c, ptr(rows), ptr(w), w.shape[1] if stride is None else stride, ptr(pub),
                             0 if pub is None else pub.shape[0], ptr(blinders), ptr(out))
    return rc, out


def _diff(got, want, t, log_ext, rho):
    return [name for name, f in CN.split(got, t, log_ext, rho).items() if f != CN.split(want, t, log_ext, rho)[name]]


@pytest.mark.parametrize("with_pi", [True, False], ids=["pi", "no_pi"])
@pytest.mark.parametrize("shape", NC.SHAPES, ids=ids)
def test_proof_bytes_against_the_oracle_and_verified(engines, oracle, shape, with_pi):
    n, t, log_ext, exps, exps_next = shape
    e = engines.bench_srs(SRS)
    d = _proof(oracle, shape, with_pi=with_pi)
    nc = d["nc"]
    circ = _create(e, nc, log_ext, want_key=True)
    try:
        assert [k.compress() for k in circ.key] == d["key48"] and circ.rho == nc.rho
        g1, g2 = _setup(oracle)
        shifts, public = [K.Scalar(k) for k in nc.circuit.ks], [K.Scalar(p) for p in d["public"]]
        proof = circ.custom_next_prove(_limbs(nc.circuit.wires, n + 5), _pub(d), n=n)  # wire stride n + 5
        want = d["proof"]
        assert len(proof) == K.circuit_custom_next_proof_size(t, log_ext, nc.rho)
        assert proof == want, _diff(proof, want, t, log_ext, nc.rho)
        assert K.circuit_custom_next_verify_proof(circ.key, n, log_ext, nc.exps, nc.exps_next, shifts, public, proof, g1, g2)
        got = K.circuit_custom_next_proof_challenges(circ.key, n, log_ext, nc.exps, nc.exps_next, shifts, public, proof)
        assert tuple(x.v for x in got) == tuple(d[k] for k in ("beta", "gamma", "alpha", "zeta", "v"))
        assert circ.custom_next_prove(_limbs(nc.circuit.wires), _pub(d)) == want  # packed wires, a second call
    finally:
        circ.close()


@pytest.mark.parametrize("shape", [NC.NEXT_ONLY, NC.WIDE], ids=ids)
def test_proof_element_is_open_sets_of_the_oracles_stack(engines, oracle, shape):
    """the proof element is bit for bit kzg_open_sets of [ r_N | wires | sigmas | z ] on {zeta}, {zeta w}, {zeta, zeta w} with gamma = v"""
    n, t, log_ext, exps, exps_next = shape
    e = engines.bench_srs(SRS)
    d = _proof(oracle, shape)
    nc = d["nc"]
    polys, set_of, sets, ys = d["stack"]
    assert set_of.count(2) == nc.rho and [len(y) for y in ys].count(2) == nc.rho
    circ = _create(e, nc, log_ext, want_key=True)
    try:
        proof = circ.custom_next_prove(_limbs(nc.circuit.wires), _pub(d))
    finally:
        circ.close()
    got_ys, w = e.open_sets_limbs(_limbs([p[:n] for p in polys]), set_of, [[K.Scalar(z) for z in s] for s in sets], K.Scalar(d["v"]))
    assert [[y.v for y in row] for row in got_ys] == [[v % R for v in row] for row in ys]
    a, b = CN.layout(t, log_ext, nc.rho)["w"]
    assert proof[a:b] == w.compress() == d["proof"][a:b]


def test_refusals_leave_the_output_untouched_and_the_context_serving(engines, oracle):
    n, t, log_ext, exps, exps_next = NC.NEXT_ONLY
    e = engines.bench_srs(SRS)
    d = _proof(oracle, NC.NEXT_ONLY)
    nc = d["nc"]
    c = nc.circuit
    wires, pub = _limbs(c.wires, n + 5), _pub(d)
    circ = _create(e, nc, log_ext, want_key=True)
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
        # blinders: next-row proofs are plain
        arr = GO.to_limbs(BO.Blinders.random(t, log_ext, 5).flat())
        refused(K.KZG_ERR_INVALID_ARG, b"not blinded", circ, wires, pub, arr)
        refused(K.KZG_ERR_INVALID_ARG, b"not blinded", circ, wires, pub, np.zeros_like(arr))
        # kzg_circuit_custom_prove on the next-row handle
        refused(K.KZG_ERR_INVALID_ARG, b"next-row terms", circ, wires, pub, fn="kzg_circuit_custom_prove")
        # a next-row term that fails ON ROW n - 1 ONLY, where the next row is row 0: the selector of that row moved (another key, the
        # same wires, every other row as before)
        s = next(s for s in range(nc.g) if any(nc.exps_next[s]))
        qx = [list(col) for col in nc.q_custom]
        qx[s][n - 1] = (qx[s][n - 1] + 1) % R
        moved = CN.NextCircuit(c, qx, nc.exps, nc.exps_next)
        rows = CN.gate_rows(moved)
        assert rows[n - 1] != 0 and not any(rows[:n - 1])
        broken = _create(e, moved, log_ext, want_key=True)
        try:
            refused(K.KZG_ERR_REMAINDER, b"not divisible", broken, wires, pub)
        finally:
            broken.close()
        # argument errors
        refused(K.KZG_ERR_INVALID_ARG, None, circ, wires, pub, stride=n - 1)
        refused(K.KZG_ERR_INVALID_ARG, None, circ, wires, np.concatenate([pub, pub[:1]]))  # n_public = n + 1
    finally:
        circ.close()


def test_kzg_circuit_prove_on_a_next_row_handle_gives_the_base_statements_status(engines, oracle):
    n, t, log_ext, exps, exps_next = NC.NEXT_ONLY
    e = engines.bench_srs(SRS)
    d = _proof(oracle, NC.NEXT_ONLY)
    nc = d["nc"]
    c = nc.circuit
    circ = _create(e, nc, log_ext, want_key=True)
    # with q_C put back so that the base gate holds, the plain proof is that of the base circuit, all custom terms ignored
    base = CO.Circuit(c.ks, c.wires, c.sigmas, c.q_lin, c.q_mul, [0] * n, c.pi)
    base.q_const = [(-v) % R for v in CO.gate_rows(base)]
    held = _create(e, CN.NextCircuit(base, nc.q_custom, nc.exps, nc.exps_next), log_ext, want_key=True)
    try:
        wires, pub = _limbs(c.wires), _pub(d)
        size = K.circuit_proof_size(t, log_ext)
        rc, out = _raw(e, circ, wires, pub, fn="kzg_circuit_prove", size=size)
        assert rc == K.KZG_ERR_REMAINDER and (out == FILL).all() and b"not divisible" in e._lib.kzg_last_error(e._h)
        plain = NC.memo("base plain proof", lambda: TR.prove(oracle, base, log_ext, BO.Blinders.zero(t, log_ext), S))
        rc, out = _raw(e, held, wires, pub, fn="kzg_circuit_prove", size=size)
        assert rc == 0 and out.tobytes() == plain["proof"]
        rc, out = _raw(e, held, wires, pub)  # the next-row statement does not hold there
        assert rc == K.KZG_ERR_REMAINDER and (out == FILL).all()
        assert circ.custom_next_prove(wires, pub) == d["proof"]
    finally:
        circ.close()
        held.close()


@pytest.mark.parametrize("shape", [NC.TINY, NC.NEXT_ONLY, NC.ACCUMULATOR], ids=ids)
def test_device_form_inside_guard_bands(engines, oracle, shape):
    import device_arena as DA
    n, t, log_ext, exps, exps_next = shape
    e = engines.bench_srs(SRS)
    d = _proof(oracle, shape)
    nc = d["nc"]
    circ = _create(e, nc, log_ext, want_key=True)
    try:
        with DA.Arena(e, seed=n + t) as arena:
            r_w = arena.region(n, t, n + 5, "wires", data=_limbs(nc.circuit.wires, n))
            arena.upload()
            proof = circ.custom_next_prove_device(r_w.ptr, _pub(d), stride=n + 5)
            arena.check_untouched()
        assert proof == d["proof"]
    finally:
        circ.close()


def test_after_a_larger_plain_proof_on_the_same_context(oracle):
    """workspaces and cross-round buffers grown by one call are reused or regrown by the next: a next-row proof at 8 rows, a plain
    proof at 2048 rows, the next-row proof again"""
    e = K.SetupArtifactsGenerator(BT.BENCH_SECRET_BE).take(2048 + 16)
    try:
        d = _proof(oracle, NC.NEXT_ONLY)
        nc = d["nc"]
        circ = _create(e, nc, NC.NEXT_ONLY[2], want_key=True)
        wires, pub = _limbs(nc.circuit.wires, 8 + 5), _pub(d)
        assert circ.custom_next_prove(wires, pub, n=8) == d["proof"]
        bc = NC.case(*NC.ONE_TILE).nc.circuit
        base = CO.Circuit(bc.ks, bc.wires, bc.sigmas, bc.q_lin, bc.q_mul, [0] * bc.n, bc.pi)
        base.q_const = [(-v) % R for v in CO.gate_rows(base)]
        big_plain = NC.memo("big plain proof", lambda: TR.prove(oracle, base, 2, BO.Blinders.zero(3, 2), S))
        big = e.circuit_create(_limbs(base.q_lin), GO.to_limbs(base.q_mul), GO.to_limbs(base.q_const), _limbs(base.sigmas),
                               [K.Scalar(k) for k in base.ks], 2, want_key=True)
        assert big.prove(_limbs(base.wires), GO.to_limbs(big_plain["public"]), None) == big_plain["proof"]
        assert circ.custom_next_prove(wires, pub, n=8) == d["proof"]
        for x in (big, circ):
            x.close()
    finally:
        e.close()


def test_on_two_device_contexts(oracle):
    n, t, log_ext, exps, exps_next = NC.NEXT_ONLY
    d = _proof(oracle, NC.NEXT_ONLY)
    cs = NC.case(*NC.NEXT_ONLY)
    nc = d["nc"]
    wires, pub = _limbs(nc.circuit.wires), _pub(d)
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(BT.BENCH_SECRET_BE, n + t + 3)
        circ = _create(rep, nc, log_ext, want_key=True)
        assert len(circ.key) == 2 * t + 2 + len(exps)
        ext = PQ.coset_extend(cs.gprime, NO.log2_exact(n) + log_ext)
        assert np.array_equal(circ.custom_next_gate(wires), GO.to_limbs(ext))
        coeffs, _ = circ.custom_next_quotient(wires, GO.to_limbs(cs.z), AL, BE, GA, public_inputs=_pi(nc.circuit))
        assert np.array_equal(coeffs, GO.to_limbs(cs.quotient[:(n << log_ext) - n]))
        assert circ.custom_next_prove(wires, pub) == d["proof"]  # forwarded to the circuit's device
        with pytest.raises(K.KzgError) as ei:
            circ.custom_next_prove_device(1 << 20, pub)  # single-device only
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        circ.close()
    finally:
        rep.close()
    split = K.Engine(devices=[0, 0])
    try:
        split.srs_generate(BT.BENCH_SECRET_BE, n)
        circ = _create(split, nc, log_ext)
        circ.key = [K.G1Point(oracle.p1_mult(oracle.p1_generator(), s % R)) for s in d["key_s"]]
        with pytest.raises(K.KzgError) as ei:
            circ.custom_next_prove(wires, pub)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG and "range-split" in str(ei.value)
        circ.close()
    finally:
        split.close()
