"""GPU: the lookup argument of a circuit whose key holds a table -- kzg_circuit_create_lookup,
kzg_circuit_lookup_columns (the test hook of k_lk_fold), kzg_circuit_lookup_quotient (the test hook of k_lk_constraints), the
table's columns through kzg_circuit_column_device, and the proof in one call, kzg_circuit_lookup_prove / _device.

Everything is compared limb for limb or byte for byte with tests/circuit_lookup_oracle.py; T also bit for bit with
kzg_circuit_quotient given the oracle's G' on the coset; every proof is verified by kzg_circuit_lookup_verify_proof.  The cases
are tests/circuit_lookup_cases.py's, each built once; there are no tolerances."""
import ctypes as C

import numpy as np
import pytest

import bigint_twin as BT
import circuit_lookup_cases as CC
import circuit_lookup_oracle as CL
import circuit_oracle as CO
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import perm_quotient_oracle as PQ

pytestmark = pytest.mark.gpu
R = CL.R
SRS = 4096
TH, BE, GA, AL = (K.Scalar(v) for v in (CC.THETA, CC.BETA, CC.GAMMA, CC.ALPHA))


def _limbs(cols, stride=None):
    """columns -> (t, stride, 4); the rows past n hold values that are not the columns'"""
    n = len(cols[0])
    stride = n if stride is None else stride
    out = np.empty((len(cols), stride, 4), dtype=np.uint64)
    for j, c in enumerate(cols):
        out[j] = GO.to_limbs(list(c) + [0xBAD + i for i in range(stride - n)])
    return out


def _create(e, lc, log_ext, stride=None, want_key=False, table=None):
    c = lc.circuit
    return e.circuit_create_lookup(_limbs(c.q_lin, stride), GO.to_limbs(c.q_mul), GO.to_limbs(c.q_const), _limbs(c.sigmas, stride),
                                   [K.Scalar(k) for k in c.ks], log_ext, _limbs(lc.table if table is None else table, stride),
                                   GO.to_limbs(lc.q_lookup), n=c.n, want_key=want_key)


def _pi(c):
    return None if c.pi is None else GO.to_limbs(c.pi)


def _full(T, n, log_ext):
    return list(T) + [0] * ((n << log_ext) - n - len(T))


def _invalid(call):
    with pytest.raises(K.KzgError) as ei:
        call()
    assert ei.value.status == K.KZG_ERR_INVALID_ARG, ei.value
    return ei.value


def _remainder(e, call):
    with pytest.raises(K.KzgError) as ei:
        call()
    assert ei.value.status == K.KZG_ERR_REMAINDER, ei.value
    assert b"not divisible" in K.load_library().kzg_last_error(e._h)


# ---- the per-proof columns and the quotient, limb for limb, at every shape -------------------------------------------------------
@pytest.mark.parametrize("n,t,c,log_ext", CC.SHAPES)
def test_columns_and_quotient_against_the_oracle(engines, n, t, c, log_ext):
    e = engines.bench_srs(SRS)
    cs = CC.case(n, t, c, log_ext)
    circ = _create(e, cs.lc, log_ext, stride=n + 3)
    try:
        wires = _limbs(cs.lc.circuit.wires, n + 5)
        f, T, m, phi, last = circ.lookup_columns(wires, TH, BE)
        assert np.array_equal(f, GO.to_limbs(cs.f)) and np.array_equal(T, GO.to_limbs(cs.T))
        assert np.array_equal(m, GO.to_limbs(cs.m)) and np.array_equal(phi, GO.to_limbs(cs.phi))
        assert last.v == 0
        coeffs, points = circ.lookup_quotient(wires, GO.to_limbs(cs.z), m, phi, AL, BE, GA, TH, public_inputs=_pi(cs.lc.circuit))
        full = _full(cs.quotient, n, log_ext)
        assert np.array_equal(coeffs, GO.to_limbs(full))
        assert len(points) == (1 << log_ext) - 1
        for k, point in enumerate(points):
            assert np.array_equal(point.p1, e.commit_limbs(GO.to_limbs(full[k * n:(k + 1) * n])).p1), k
        # bit for bit what kzg_circuit_quotient returns given the oracle's G' on the coset (the handle's table is ignored there)
        ext = PQ.coset_extend(cs.gprime or [0], NO.log2_exact(n) + log_ext)
        old_c, old_p = circ.quotient(wires, GO.to_limbs(cs.z), AL, BE, GA, public_inputs=_pi(cs.lc.circuit), gate=GO.to_limbs(ext))
        assert np.array_equal(coeffs, old_c)
        assert all(np.array_equal(x.p1, y.p1) for x, y in zip(points, old_p))
    finally:
        circ.close()


# ---- the key: commitments and the resident table ---------------------------------------------------------------------------------
def test_key_commitments_and_resident_table_columns(engines):
    n, t, c, log_ext = 256, 3, 2, 2
    N = n << log_ext
    e = engines.bench_srs(SRS)
    cs = CC.case(n, t, c, log_ext)
    circ = _create(e, cs.lc, log_ext, stride=n + 3, want_key=True)
    plain = e.circuit_create(_limbs(cs.lc.circuit.q_lin), GO.to_limbs(cs.lc.circuit.q_mul), GO.to_limbs(cs.lc.circuit.q_const),
                             _limbs(cs.lc.circuit.sigmas), [K.Scalar(k) for k in cs.lc.circuit.ks], log_ext)
    try:
        cols = cs.lc.key_columns()
        assert len(circ.key) == 2 * t + c + 3 and circ.c == c
        for j, col in enumerate(cols):  # kzg_circuit_create's order, then tab_0.., q_K
            assert np.array_equal(circ.key[j].p1, e.commit_evaluations_limbs(GO.to_limbs(col)).p1), j
        for j in range(2 * t + 2):
            assert np.array_equal(circ.key[j].p1, plain.key[j].p1), j
        which = [K.KZG_CIRCUIT_COL_TABLE + j for j in range(c)] + [K.KZG_CIRCUIT_COL_QLOOKUP]
        ext = e.coset_extend_limbs(_limbs(cols[2 * t + 2:]), NO.log2_exact(N))
        lib = K.load_library()

        def down(p, rows):
            got = np.zeros((rows, 4), dtype=np.uint64)
            assert lib.kzg_dev_download(e._h, got.ctypes.data, C.c_void_p(p), rows * 32) == 0
            return got
        for j, w in enumerate(which):
            col = cols[2 * t + 2 + j]
            p, ln = circ.column_device(w, K.KZG_CIRCUIT_VALUES)
            assert ln == n and np.array_equal(down(p, n), GO.to_limbs(col)), j
            p, ln = circ.column_device(w, K.KZG_CIRCUIT_COEFFS)
            assert ln == n and np.array_equal(down(p, n), GO.to_limbs(NO.intt(col))), j
            p, ln = circ.column_device(w, K.KZG_CIRCUIT_COSET)
            assert ln == N and np.array_equal(down(p, N), ext[j]), j
        # behind the sigmas, contiguous
        p0, _ = circ.column_device(K.KZG_CIRCUIT_COL_QLIN, K.KZG_CIRCUIT_COEFFS)
        pt, _ = circ.column_device(K.KZG_CIRCUIT_COL_TABLE, K.KZG_CIRCUIT_COEFFS)
        assert pt == p0 + (2 * t + 2) * n * 32
        for circuit, w in ((circ, K.KZG_CIRCUIT_COL_TABLE + c), (plain, K.KZG_CIRCUIT_COL_TABLE), (plain, K.KZG_CIRCUIT_COL_QLOOKUP)):
            _invalid(lambda: circuit.column_device(w, K.KZG_CIRCUIT_VALUES))
        # a circuit without a table has no lookup columns and no lookup quotient
        wires = _limbs(cs.lc.circuit.wires)
        _invalid(lambda: plain.lookup_columns(wires, TH, BE))
        _invalid(lambda: plain.lookup_quotient(wires, GO.to_limbs(cs.z), GO.to_limbs(cs.m), GO.to_limbs(cs.phi), AL, BE, GA, TH))
    finally:
        circ.close()
        plain.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_a_tuple_outside_the_table_names_its_row_and_the_context_goes_on(engines):
    n, t, c, log_ext = 8, 3, 3, 2
    e = engines.bench_srs(SRS)
    cs = CC.case(n, t, c, log_ext)
    circ = _create(e, cs.lc, log_ext)
    try:
        row = max(i for i in range(n) if cs.lc.q_lookup[i])
        bad = [list(col) for col in cs.lc.circuit.wires]
        bad[c - 1][row] = (bad[c - 1][row] + 1) % R
        assert CL.columns(cs.lc, CC.THETA, CC.BETA, wires=bad)[5] == row
        err = _invalid(lambda: circ.lookup_columns(_limbs(bad), TH, BE))
        assert err.bad_row == row and b"in no table row" in K.load_library().kzg_last_error(e._h)
        f, T, m, phi, last = circ.lookup_columns(_limbs(cs.lc.circuit.wires), TH, BE)  # the next call succeeds
        assert np.array_equal(phi, GO.to_limbs(cs.phi)) and last.v == 0
    finally:
        circ.close()


def test_a_table_without_the_zero_tuple_beside_an_unselected_row(engines):
    n, t, c, log_ext = 8, 3, 3, 2
    e = engines.bench_srs(SRS)
    cs = CC.case(n, t, c, log_ext)
    some = next(i for i in range(n) if cs.lc.q_lookup[i])
    tup = [cs.lc.circuit.wires[j][some] for j in range(c)]
    table = [[tup[j] if all(col[i] == 0 for col in cs.lc.table) else cs.lc.table[j][i] for i in range(n)] for j in range(c)]
    assert CL.columns(cs.lc, CC.THETA, CC.BETA, table=table)[5] == cs.lc.q_lookup.index(0)
    circ = _create(e, cs.lc, log_ext, table=table)
    try:
        err = _invalid(lambda: circ.lookup_columns(_limbs(cs.lc.circuit.wires), TH, BE))
        assert err.bad_row == cs.lc.q_lookup.index(0)
    finally:
        circ.close()


def test_a_zero_denominator_names_its_row(engines):
    n, t, c, log_ext = 8, 3, 3, 2
    e = engines.bench_srs(SRS)
    cs = CC.case(n, t, c, log_ext)
    circ = _create(e, cs.lc, log_ext)
    try:
        row = 4  # a selected row: f there is not zero
        assert cs.lc.q_lookup[row] and cs.f[row]
        beta = (-cs.f[row]) % R
        want = min(i for i in range(n) if (beta + cs.f[i]) % R == 0 or (beta + cs.T[i]) % R == 0)
        err = _invalid(lambda: circ.lookup_columns(_limbs(cs.lc.circuit.wires), TH, K.Scalar(beta)))
        assert err.bad_row == want and b"denominator" in K.load_library().kzg_last_error(e._h)
    finally:
        circ.close()


def test_false_columns_leave_a_remainder(engines):
    n, t, c, log_ext = 8, 3, 3, 2
    e = engines.bench_srs(SRS)
    cs = CC.case(n, t, c, log_ext)
    lcirc = cs.lc.circuit
    circ = _create(e, cs.lc, log_ext)
    try:
        wires, z, pi = _limbs(lcirc.wires), GO.to_limbs(cs.z), _pi(lcirc)
        run = lambda w=wires, zz=z, m=cs.m, phi=cs.phi: circ.lookup_quotient(w, zz, GO.to_limbs(m), GO.to_limbs(phi), AL, BE, GA, TH,
                                                                             public_inputs=pi, want_commitments=False)
        coeffs, _ = run()
        assert np.array_equal(coeffs, GO.to_limbs(_full(cs.quotient, n, log_ext)))
        m2, phi2 = list(cs.m), list(cs.phi)
        m2[2] = (m2[2] + 1) % R
        phi2[3] = (phi2[3] + 1) % R
        for kw in ({"m": m2}, {"phi": phi2}):
            assert CL.remainder(cs.lc, cs.z, CC.THETA, CC.BETA, CC.GAMMA, CC.ALPHA, kw.get("m", cs.m), kw.get("phi", cs.phi)) != []
            _remainder(e, lambda: run(**kw))
        # a broken gate row (a wire no lookup reads: the columns stay those of the wires) and a broken copy constraint (z of other wires)
        bad = [list(col) for col in lcirc.wires]
        row = cs.lc.q_lookup.index(0)
        bad[0][row] = (bad[0][row] + 1) % R
        _remainder(e, lambda: run(w=_limbs(bad)))
        z2 = list(cs.z)
        z2[n - 1] = (z2[n - 1] + 1) % R
        _remainder(e, lambda: run(zz=GO.to_limbs(z2)))
        coeffs, _ = run()  # the context goes on
        assert np.array_equal(coeffs, GO.to_limbs(_full(cs.quotient, n, log_ext)))
    finally:
        circ.close()


def test_shape_rules_and_arguments(engines):
    e = engines.bench_srs(SRS)
    cs = CC.case(8, 3, 3, 2)
    lc, c = cs.lc, cs.lc.circuit
    ok = _create(e, lc, 2)
    ok.close()
    # c > t, c = 0 (no table column), e < 4 cannot hold t = 3; 3 t + e + c + 5 > 32 at t = 6, e = 8, c = 2
    args = lambda t, n=8: (_limbs(c.q_lin[:1] * t), GO.to_limbs(c.q_mul), GO.to_limbs(c.q_const), _limbs(c.sigmas[:1] * t),
                           [K.Scalar(k) for k in GO.shifts(t)])
    _invalid(lambda: e.circuit_create_lookup(*args(2), 2, _limbs(lc.table[:1] * 3), GO.to_limbs(lc.q_lookup), want_key=False))
    _invalid(lambda: e.circuit_create_lookup(*args(2), 1, _limbs(lc.table[:1]), GO.to_limbs(lc.q_lookup), want_key=False))
    _invalid(lambda: e.circuit_create_lookup(*args(6), 3, _limbs(lc.table[:1] * 2), GO.to_limbs(lc.q_lookup), want_key=False))
    fits = e.circuit_create_lookup(*args(6), 3, _limbs(lc.table[:1]), GO.to_limbs(lc.q_lookup), want_key=False)
    fits.close()


# ---- a replicated two-device context ---------------------------------------------------------------------------------------------
def test_on_a_replicated_two_device_context():
    n, t, c, log_ext = 8, 3, 3, 2
    cs = CC.case(n, t, c, log_ext)
    e = K.Engine(devices=[0, 0], replicate=True)
    try:
        e.srs_generate(BT.BENCH_SECRET_BE, n)
        circ = _create(e, cs.lc, log_ext, want_key=True)
        assert len(circ.key) == 2 * t + c + 3
        wires = _limbs(cs.lc.circuit.wires)
        f, T, m, phi, last = circ.lookup_columns(wires, TH, BE)
        assert np.array_equal(m, GO.to_limbs(cs.m)) and np.array_equal(phi, GO.to_limbs(cs.phi))
        coeffs, points = circ.lookup_quotient(wires, GO.to_limbs(cs.z), m, phi, AL, BE, GA, TH, public_inputs=_pi(cs.lc.circuit))
        assert np.array_equal(coeffs, GO.to_limbs(_full(cs.quotient, n, log_ext)))
        circ.close()
    finally:
        e.close()


# ---- the proof in one call: kzg_circuit_lookup_prove / _device --------------------------------------------------------------------
S = BT.fr_from_be_bytes(BT.BENCH_SECRET_BE)
FILL = 0x5A


def _proof(oracle, n, t, c, log_ext, with_pi=True):
    """tests/circuit_lookup_oracle.py's proof under the bench secret, computed once"""
    return CC.memo(("bench proof", n, t, c, log_ext, with_pi), lambda: CL.prove(oracle, CC.case(n, t, c, log_ext, with_pi).lc, log_ext, S))


def _setup(oracle):
    """[s^0]G1 and [s^j]G2, j <= 2, of the bench secret"""
    return CC.memo("setup", lambda: (np.stack([oracle.p1_generator()]), np.stack([K.srs_g2_at(BT.BENCH_SECRET_BE, j) for j in range(3)])))


def _pub(d):
    return GO.to_limbs(d["public"]) if d["public"] else None


def _raw(e, circ, wires, pub, fn="kzg_circuit_lookup_prove", stride=None, n_public=None):
    """the C call on a pre-filled output: (status, the output bytes, bad_row)"""
    rows = np.ascontiguousarray(np.stack([p.p1 for p in circ.key]), dtype=np.uint64)
    out = np.full(K.circuit_lookup_proof_size(circ.t, circ.log_ext, circ.c), FILL, dtype=np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    w = np.ascontiguousarray(wires)
    bad = C.c_size_t(12345)
    rc = getattr(e._lib, fn)(e._h, circ._c, ptr(rows), ptr(w), w.shape[1] if stride is None else stride, ptr(pub),
                             (0 if pub is None else pub.shape[0]) if n_public is None else n_public, ptr(out), C.byref(bad))
    return rc, out, bad.value


@pytest.mark.parametrize("with_pi", [True, False], ids=["pi", "no_pi"])
@pytest.mark.parametrize("n,t,c,log_ext", CC.SHAPES)
def test_proof_bytes_against_the_oracle_and_verified(engines, oracle, n, t, c, log_ext, with_pi):
    e = engines.bench_srs(SRS)
    d = _proof(oracle, n, t, c, log_ext, with_pi)
    lc = d["lc"]
    circ = _create(e, lc, log_ext, want_key=True)
    try:
        assert [k.compress() for k in circ.key] == d["key48"]
        proof = circ.lookup_prove(_limbs(lc.circuit.wires, n + 5), _pub(d), n=n)
        want = d["proof"]
        assert proof == want, [name for name, f in CL.split(proof, t, log_ext, c).items() if f != CL.split(want, t, log_ext, c)[name]]
        g1, g2 = _setup(oracle)
        shifts, public = [K.Scalar(k) for k in lc.circuit.ks], [K.Scalar(p) for p in d["public"]]
        assert K.circuit_lookup_verify_proof(circ.key, n, log_ext, c, shifts, public, proof, g1, g2)
        got = K.circuit_lookup_proof_challenges(circ.key, n, log_ext, c, shifts, public, proof)
        assert tuple(x.v for x in got) == tuple(d[k] for k in ("theta", "beta", "gamma", "alpha", "zeta", "v"))
        assert circ.lookup_prove(_limbs(lc.circuit.wires), _pub(d)) == want  # packed wires, a second call
    finally:
        circ.close()


def test_a_plain_proof_on_the_lookup_circuits_handle(engines, oracle):
    import blind_oracle as BO
    import transcript_oracle as TR
    n, t, c, log_ext = 8, 3, 3, 2
    e = engines.bench_srs(SRS)
    d = _proof(oracle, n, t, c, log_ext)
    lc = d["lc"]
    plain = CC.memo("plain proof", lambda: TR.prove(oracle, lc.circuit, log_ext, BO.Blinders.zero(t, log_ext), S))
    circ = _create(e, lc, log_ext, want_key=True)
    try:
        assert circ.prove(_limbs(lc.circuit.wires, n + 5), _pub(d), None, n=n) == plain["proof"]  # the table is ignored
        assert circ.lookup_prove(_limbs(lc.circuit.wires), _pub(d)) == d["proof"]
        g1, g2 = _setup(oracle)
        shifts, public = [K.Scalar(k) for k in lc.circuit.ks], [K.Scalar(p) for p in d["public"]]
        assert K.circuit_verify_proof(circ.key[:2 * t + 2], n, log_ext, shifts, public, plain["proof"], g1, g2)
    finally:
        circ.close()


def test_prover_statuses_leave_the_output_untouched_and_the_context_serving(engines, oracle):
    n, t, c, log_ext = 8, 3, 3, 2
    e = engines.bench_srs(SRS)
    d = _proof(oracle, n, t, c, log_ext)
    lc = d["lc"]
    lcirc = lc.circuit
    wires, pub = _limbs(lcirc.wires, n + 5), _pub(d)
    circ = _create(e, lc, log_ext, want_key=True)
    # the same circuit with one row's constant changed (the gate fails there), and with a table that lost the zero tuple
    q_const = list(lcirc.q_const)
    q_const[3] = (q_const[3] + 1) % R
    broken_lc = CL.LookupCircuit(CO.Circuit(lcirc.ks, lcirc.wires, lcirc.sigmas, lcirc.q_lin, lcirc.q_mul, q_const, lcirc.pi), lc.table, lc.q_lookup)
    broken = _create(e, broken_lc, log_ext, want_key=True)
    some = next(i for i in range(n) if lc.q_lookup[i])
    tup = [lcirc.wires[j][some] for j in range(c)]
    no_zero = [[tup[j] if all(col[i] == 0 for col in lc.table) else lc.table[j][i] for i in range(n)] for j in range(c)]
    zeroless = _create(e, lc, log_ext, want_key=True, table=no_zero)
    plain = e.circuit_create(_limbs(lcirc.q_lin), GO.to_limbs(lcirc.q_mul), GO.to_limbs(lcirc.q_const), _limbs(lcirc.sigmas),
                             [K.Scalar(k) for k in lcirc.ks], log_ext)
    plain.key, plain.c = circ.key, c
    try:
        def good():
            rc, out, bad = _raw(e, circ, wires, pub)
            assert rc == 0 and out.tobytes() == d["proof"] and bad == C.c_size_t(-1).value

        def refused(status, message, bad_row, *args, **kw):
            rc, out, bad = _raw(e, *args, **kw)
            assert rc == status and (out == FILL).all(), (rc, message)
            assert bad == (C.c_size_t(-1).value if bad_row is None else bad_row), (bad, bad_row)
            if message:
                assert message in e._lib.kzg_last_error(e._h), e._lib.kzg_last_error(e._h)
            good()

        good()
        # a wire tuple outside the table: the least such row
        row = max(i for i in range(n) if lc.q_lookup[i])
        moved = wires.copy()
        moved[c - 1, row] = GO.to_limbs([(lcirc.wires[c - 1][row] + 1) % R])[0]
        refused(K.KZG_ERR_REMAINDER, b"row %d" % row, row, circ, moved, pub)
        # a table without the zero tuple beside a q_K = 0 row
        refused(K.KZG_ERR_REMAINDER, b"row %d" % lc.q_lookup.index(0), lc.q_lookup.index(0), zeroless, wires, pub)
        # an unsatisfied gate row; a broken copy constraint (a wire no lookup reads: the lookup holds, z does not return to one)
        refused(K.KZG_ERR_REMAINDER, b"not divisible", None, broken, wires, pub)
        free = lc.q_lookup.index(0)
        moved = wires.copy()
        moved[0, free] = GO.to_limbs([(lcirc.wires[0][free] + 1) % R])[0]
        refused(K.KZG_ERR_REMAINDER, b"z_n != 1", None, circ, moved, pub)
        # argument errors, in the header's order
        not_fr = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
        refused(K.KZG_ERR_INVALID_ARG, b"without a lookup table", None, plain, wires, pub)
        refused(K.KZG_ERR_INVALID_ARG, None, None, circ, wires, pub, stride=n - 1)
        refused(K.KZG_ERR_INVALID_ARG, None, None, circ, wires, np.concatenate([pub, pub[:1]]))  # n_public = n + 1
        bad_pub = pub.copy()
        bad_pub[n - 1] = not_fr
        refused(K.KZG_ERR_INVALID_ARG, b"public input is not below r", None, circ, wires, bad_pub)
        other = engines.bench_srs(n)
        rc, out, _ = _raw(other, circ, wires, pub)  # a circuit of another context
        assert rc == K.KZG_ERR_INVALID_ARG and (out == FILL).all()
        good()
        bare = K.Engine(0)  # no SRS
        try:
            nokey = _create(bare, lc, log_ext)
            nokey.key = circ.key
            rc, out, _ = _raw(bare, nokey, wires, pub)
            assert rc == K.KZG_ERR_NO_SRS and (out == FILL).all()
            nokey.close()
        finally:
            bare.close()
        short = engines.bench_srs(n // 2)  # fewer than n points
        nokey = _create(short, lc, log_ext)
        nokey.key = circ.key
        rc, out, _ = _raw(short, nokey, wires, pub)
        assert rc == K.KZG_ERR_DEGREE_TOO_HIGH and (out == FILL).all()
        nokey.close()
    finally:
        for x in (circ, broken, zeroless, plain):
            x.close()


@pytest.mark.parametrize("n,t,c,log_ext", [(8, 3, 3, 2), (256, 3, 2, 2), (2, 3, 2, 2)])
def test_device_form_inside_guard_bands(engines, oracle, n, t, c, log_ext):
    import device_arena as DA
    e = engines.bench_srs(SRS)
    d = _proof(oracle, n, t, c, log_ext)
    lc = d["lc"]
    circ = _create(e, lc, log_ext, want_key=True)
    try:
        with DA.Arena(e, seed=n + t) as arena:
            r_w = arena.region(n, t, n + 5, "wires", data=_limbs(lc.circuit.wires, n))
            arena.upload()
            proof = circ.lookup_prove_device(r_w.ptr, _pub(d), stride=n + 5)
            arena.check_untouched()
        assert proof == d["proof"]
    finally:
        circ.close()


def test_after_a_larger_plain_proof_on_the_same_context(oracle):
    """workspaces and cross-round buffers grown by one call are reused or regrown by the next: a lookup proof at 8 rows, a plain
    proof at 2048, the lookup proof again"""
    import blind_oracle as BO
    import transcript_oracle as TR
    e = K.SetupArtifactsGenerator(BT.BENCH_SECRET_BE).take(2048)
    try:
        d = _proof(oracle, 8, 3, 3, 2)
        lc = d["lc"]
        circ = _create(e, lc, 2, want_key=True)
        wires, pub = _limbs(lc.circuit.wires, 8 + 5), _pub(d)
        assert circ.lookup_prove(wires, pub, n=8) == d["proof"]
        big_lc = CC.case(2048, 3, 2, 2).lc
        big_plain = CC.memo("big plain proof", lambda: TR.prove(oracle, big_lc.circuit, 2, BO.Blinders.zero(3, 2), S))
        big = _create(e, big_lc, 2, want_key=True)
        assert big.prove(_limbs(big_lc.circuit.wires), GO.to_limbs(big_plain["public"]), None) == big_plain["proof"]
        assert circ.lookup_prove(wires, pub, n=8) == d["proof"]
        assert big.lookup_prove(_limbs(big_lc.circuit.wires), GO.to_limbs(big_plain["public"])) == _proof(oracle, 2048, 3, 2, 2)["proof"]
        assert circ.lookup_prove(wires, pub, n=8) == d["proof"]
        big.close()
        circ.close()
    finally:
        e.close()


def test_proofs_on_two_device_contexts(oracle):
    n, t, c, log_ext = 8, 3, 3, 2
    d = _proof(oracle, n, t, c, log_ext)
    lc = d["lc"]
    wires, pub = _limbs(lc.circuit.wires), _pub(d)
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(BT.BENCH_SECRET_BE, n)
        circ = _create(rep, lc, log_ext, want_key=True)
        assert circ.lookup_prove(wires, pub) == d["proof"]  # forwarded to the circuit's device
        with pytest.raises(K.KzgError) as ei:
            circ.lookup_prove_device(1 << 20, pub)  # single-device only
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        circ.close()
    finally:
        rep.close()
    split = K.Engine(devices=[0, 0])
    try:
        split.srs_generate(BT.BENCH_SECRET_BE, n)
        circ = _create(split, lc, log_ext)
        circ.key = [K.G1Point(oracle.p1_mult(oracle.p1_generator(), s % R)) for s in d["key_s"]]
        with pytest.raises(K.KzgError) as ei:
            circ.lookup_prove(wires, pub)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG and "range-split" in str(ei.value)
        circ.close()
    finally:
        split.close()
