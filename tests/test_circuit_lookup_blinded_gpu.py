"""GPU: zero-knowledge lookup proofs -- kzg_circuit_lookup_quotient_blinded (the test hook of T~) and the
proof in one call, kzg_circuit_lookup_prove_blinded / _device.

T~ is compared limb for limb, its chunks' commitments bit for bit and the proof byte for byte with
tests/circuit_lookup_blind_oracle.py under the bench secret; every proof is verified by the EXISTING kzg_circuit_lookup_verify_proof.
The cases are circuit_lookup_cases' with a table of full degree (circuit_lookup_blind_oracle.case), each built once; there are no
tolerances.  Shapes (n, t, c, log_ext): (4, 2, 1, 2) where the lookup's term sets T~'s degree, (8, 3, 3, 2) where the permutation's
does, (1, 2, 1, 3) with one opening point, (2, 3, 2, 3) where the patches' index ranges overlap, (256, 3, 2, 2) and (4096, 2, 1, 2)
on the transform paths of section 4.26's cases, and (64, 6, 1, 3) with 16 records of the tail kernel at zeta."""
import ctypes as C

import numpy as np
import pytest

import bigint_twin as BT
import circuit_custom_cases as XC
import circuit_lookup_blind_oracle as LB
import circuit_lookup_cases as CC
import circuit_lookup_oracle as CL
import circuit_next_cases as NC
import circuit_oracle as CO
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import test_circuit_custom_gpu as XG  # the other kinds' oracle proofs under the bench secret (shared, computed once) and handles
import test_circuit_next_gpu as NG
import test_circuit_proof_gpu as HC

pytestmark = pytest.mark.gpu
R = CL.R
SRS = 4096 + 2 + 3  # n + t + 3 at the largest shape
SHAPES = [(4, 2, 1, 2), (8, 3, 3, 2), (1, 2, 1, 3), (2, 3, 2, 3), (256, 3, 2, 2), (4096, 2, 1, 2), (64, 6, 1, 3)]
S = BT.fr_from_be_bytes(BT.BENCH_SECRET_BE)
FILL = 0x5A
NOT_FR = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def _limbs(cols, stride=None):
    """columns -> (t, stride, 4); the rows past n hold values that are not the columns'"""
    n = len(cols[0])
    stride = n if stride is None else stride
    out = np.empty((len(cols), stride, 4), dtype=np.uint64)
    for j, c in enumerate(cols):
        out[j] = GO.to_limbs(list(c) + [0xBAD + i for i in range(stride - n)])
    return out


def _create(e, lc, log_ext, want_key=True, table=None):
    c = lc.circuit
    return e.circuit_create_lookup(_limbs(c.q_lin), GO.to_limbs(c.q_mul), GO.to_limbs(c.q_const), _limbs(c.sigmas),
                                   [K.Scalar(k) for k in c.ks], log_ext, _limbs(lc.table if table is None else table),
                                   GO.to_limbs(lc.q_lookup), n=c.n, want_key=want_key)


def _blinders(t, log_ext, seed):
    return LB.Blinders.random(t, log_ext, seed)


def _proof(oracle, n, t, c, log_ext, with_pi=True, seed=None):
    """the oracle's blinded proof under the bench secret, computed once"""
    seed = n + t if seed is None else seed
    return CC.memo(("bench blinded proof", n, t, c, log_ext, with_pi, seed),
                   lambda: LB.prove(oracle, LB.case(n, t, c, log_ext, with_pi).lc, log_ext, _blinders(t, log_ext, seed), S))


def _setup(oracle):
    """[s^0]G1 and [s^j]G2, j <= 2, of the bench secret"""
    return CC.memo("setup", lambda: (np.stack([oracle.p1_generator()]), np.stack([K.srs_g2_at(BT.BENCH_SECRET_BE, j) for j in range(3)])))


def _pub(d):
    return GO.to_limbs(d["public"]) if d["public"] else None


def _verified(oracle, circ, lc, log_ext, public, proof):
    g1, g2 = _setup(oracle)
    return K.circuit_lookup_verify_proof(circ.key, lc.n, log_ext, lc.c, [K.Scalar(k) for k in lc.circuit.ks],
                                         [K.Scalar(p) for p in public], proof, g1, g2)


def _raw(e, circ, wires, pub, bl, fn="kzg_circuit_lookup_prove_blinded", stride=None, n_public=None):
    """the C call on a pre-filled output: (status, the output bytes, bad_row)"""
    rows = np.ascontiguousarray(np.stack([p.p1 for p in circ.key]), dtype=np.uint64)
    out = np.full(K.circuit_lookup_proof_size(circ.t, circ.log_ext, circ.c), FILL, dtype=np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    w = np.ascontiguousarray(wires)
    b = None if bl is None else np.ascontiguousarray(bl, dtype=np.uint64)
    bad = C.c_size_t(12345)
    more = () if fn == "kzg_circuit_lookup_prove" else (ptr(b),)  # (the plain prover, for comparison, takes no blinders)
    rc = getattr(e._lib, fn)(e._h, circ._c, ptr(rows), ptr(w), w.shape[1] if stride is None else stride, ptr(pub),
                             (0 if pub is None else pub.shape[0]) if n_public is None else n_public, *more, ptr(out), C.byref(bad))
    return rc, out, bad.value


# ---- T~ and its chunks' commitments, at every shape --------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t,c,log_ext", SHAPES)
def test_quotient_and_chunk_commitments_against_the_oracle(engines, oracle, n, t, c, log_ext):
    e = engines.bench_srs(SRS)
    d = _proof(oracle, n, t, c, log_ext)
    lc, bl = d["lc"], GO.to_limbs(d["bl"].flat())
    assert K.circuit_lookup_blinded_sizes(n, t, log_ext, c) == (bl.shape[0], len(d["T"]))
    circ = _create(e, lc, log_ext, want_key=False)
    try:
        ch = [K.Scalar(d[k]) for k in ("alpha", "beta", "gamma", "theta")]
        coeffs, points = circ.lookup_quotient_blinded(_limbs(lc.circuit.wires, n + 5), GO.to_limbs(d["z"]), GO.to_limbs(d["m"]),
                                                      GO.to_limbs(d["phi"]), *ch, bl, public_inputs=_pi(lc.circuit), n=n)
        assert np.array_equal(coeffs, GO.to_limbs(d["T"]))
        D = LB.keep(n, t)
        assert not coeffs[D:].any() and (n <= 2 or coeffs[D - 1].any())
        assert len(points) == (1 << log_ext) - 1
        for k, point in enumerate(points):
            assert np.array_equal(point.p1, e.commit_limbs(GO.to_limbs(d["chunks"][k])).p1), k
    finally:
        circ.close()


def _pi(c):
    return None if c.pi is None else GO.to_limbs(c.pi)


# ---- the proof in one call -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_pi", [True, False], ids=["pi", "no_pi"])
@pytest.mark.parametrize("n,t,c,log_ext", SHAPES)
def test_proof_bytes_against_the_oracle_and_verified(engines, oracle, n, t, c, log_ext, with_pi):
    e = engines.bench_srs(SRS)
    d = _proof(oracle, n, t, c, log_ext, with_pi)
    lc, bl = d["lc"], GO.to_limbs(d["bl"].flat())
    circ = _create(e, lc, log_ext)
    try:
        assert [k.compress() for k in circ.key] == d["key48"]
        proof = circ.lookup_prove_blinded(_limbs(lc.circuit.wires, n + 5), bl, _pub(d), n=n)
        want = d["proof"]
        assert proof == want, [name for name, f in CL.split(proof, t, log_ext, c).items() if f != CL.split(want, t, log_ext, c)[name]]
        assert _verified(oracle, circ, lc, log_ext, d["public"], proof)
        got = K.circuit_lookup_proof_challenges(circ.key, n, log_ext, c, [K.Scalar(k) for k in lc.circuit.ks],
                                                [K.Scalar(p) for p in d["public"]], proof)
        assert tuple(x.v for x in got) == tuple(d[k] for k in ("theta", "beta", "gamma", "alpha", "zeta", "v"))
    finally:
        circ.close()


@pytest.mark.parametrize("n,t,c,log_ext", SHAPES)
def test_all_blinders_zero_give_the_bytes_of_the_plain_prover(engines, n, t, c, log_ext):
    e = engines.bench_srs(SRS)
    lc = LB.case(n, t, c, log_ext).lc
    circ = _create(e, lc, log_ext)
    try:
        wires, pub = _limbs(lc.circuit.wires, n + 5), _pi(lc.circuit)
        zero = np.zeros((2 * t + (1 << log_ext) + 6, 4), dtype=np.uint64)
        assert circ.lookup_prove_blinded(wires, zero, pub, n=n) == circ.lookup_prove(wires, pub, n=n)
    finally:
        circ.close()


def test_two_blinder_sets_on_one_witness(engines, oracle):
    n, t, c, log_ext = 8, 3, 3, 2
    e = engines.bench_srs(SRS)
    lc = LB.case(n, t, c, log_ext).lc
    circ = _create(e, lc, log_ext)
    try:
        wires, pub = _limbs(lc.circuit.wires), _pi(lc.circuit)
        a = circ.lookup_prove_blinded(wires, K.circuit_lookup_blinders(t, log_ext), pub)
        b = circ.lookup_prove_blinded(wires, K.circuit_lookup_blinders(t, log_ext), pub)
        plain = circ.lookup_prove(wires, pub)
        fa, fb, fp = (CL.split(x, t, log_ext, c) for x in (a, b, plain))
        for name in ("wires", "m", "z", "phi", "chunks"):
            for i in range(0, len(fa[name]), 48):
                assert len({fa[name][i:i + 48], fb[name][i:i + 48], fp[name][i:i + 48]}) == 3, (name, i)
        for j in range(t):  # abar_j
            assert len({fa["evals"][32 * j:32 * j + 32], fb["evals"][32 * j:32 * j + 32], fp["evals"][32 * j:32 * j + 32]}) == 3, j
        assert len({fa["evals"][-32:], fb["evals"][-32:], fp["evals"][-32:]}) == 3  # phi~(zeta w)
        public = [] if lc.circuit.pi is None else lc.circuit.pi
        for proof in (a, b, plain):
            assert _verified(oracle, circ, lc, log_ext, public, proof)
    finally:
        circ.close()


@pytest.mark.parametrize("n,t,c,log_ext", [(8, 3, 3, 2), (256, 3, 2, 2), (2, 3, 2, 3)])
def test_device_form_inside_guard_bands(engines, oracle, n, t, c, log_ext):
    import device_arena as DA
    e = engines.bench_srs(SRS)
    d = _proof(oracle, n, t, c, log_ext)
    lc = d["lc"]
    circ = _create(e, lc, log_ext)
    try:
        with DA.Arena(e, seed=n + t) as arena:
            r_w = arena.region(n, t, n + 5, "wires", data=_limbs(lc.circuit.wires, n))
            arena.upload()
            proof = circ.lookup_prove_blinded_device(r_w.ptr, GO.to_limbs(d["bl"].flat()), _pub(d), stride=n + 5)
            arena.check_untouched()
        assert proof == d["proof"]
    finally:
        circ.close()


# ---- statuses ------------------------------------------------------------------------------------------------------------------------
def test_prover_statuses_leave_the_output_untouched_and_the_context_serving(engines, oracle):
    n, t, c, log_ext = 8, 3, 3, 2
    e = engines.bench_srs(SRS)
    d = _proof(oracle, n, t, c, log_ext)
    lc = d["lc"]
    lcirc = lc.circuit
    wires, pub, bl = _limbs(lcirc.wires, n + 5), _pub(d), GO.to_limbs(d["bl"].flat())
    circ = _create(e, lc, log_ext)
    q_const = list(lcirc.q_const)
    q_const[3] = (q_const[3] + 1) % R
    broken_lc = CL.LookupCircuit(CO.Circuit(lcirc.ks, lcirc.wires, lcirc.sigmas, lcirc.q_lin, lcirc.q_mul, q_const, lcirc.pi), lc.table, lc.q_lookup)
    broken = _create(e, broken_lc, log_ext)
    plain = e.circuit_create(_limbs(lcirc.q_lin), GO.to_limbs(lcirc.q_mul), GO.to_limbs(lcirc.q_const), _limbs(lcirc.sigmas),
                             [K.Scalar(k) for k in lcirc.ks], log_ext)
    plain.key, plain.c = circ.key, c
    small_lc = CC.case(2, 3, 2, 2).lc  # a lookup circuit's shape that the blinded forms refuse
    small = _create(e, small_lc, 2)
    try:
        def good():
            rc, out, bad = _raw(e, circ, wires, pub, bl)
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
        refused(K.KZG_ERR_REMAINDER, b"row %d" % row, row, circ, moved, pub, bl)
        # an unsatisfied gate row; a broken copy constraint
        refused(K.KZG_ERR_REMAINDER, b"not divisible", None, broken, wires, pub, bl)
        free = lc.q_lookup.index(0)
        moved = wires.copy()
        moved[0, free] = GO.to_limbs([(lcirc.wires[0][free] + 1) % R])[0]
        refused(K.KZG_ERR_REMAINDER, b"z_n != 1", None, circ, moved, pub, bl)
        # argument errors
        refused(K.KZG_ERR_INVALID_ARG, None, None, circ, wires, pub, None)  # blinders are required
        refused(K.KZG_ERR_INVALID_ARG, b"without a lookup table", None, plain, wires, pub, bl)
        refused(K.KZG_ERR_INVALID_ARG, None, None, circ, wires, pub, bl, stride=n - 1)
        bad_pub = pub.copy()
        bad_pub[n - 1] = NOT_FR
        refused(K.KZG_ERR_INVALID_ARG, b"public input is not below r", None, circ, wires, bad_pub, bl)
        # the shape rule, then the blinders: each group's last entry
        sw = _limbs(small_lc.circuit.wires)
        refused(K.KZG_ERR_INVALID_ARG, b"the blinded lookup quotient needs", None, small, sw, _pi(small_lc.circuit),
                np.zeros((2 * 3 + 4 + 6, 4), dtype=np.uint64))
        rc, out, _ = _raw(e, small, sw, _pi(small_lc.circuit), None, fn="kzg_circuit_lookup_prove")
        assert rc == 0  # (the plain prover takes the shape)
        e_ = 1 << log_ext
        for index in (2 * t - 1, 2 * t + 2, 2 * t + 3 + e_ - 3, 2 * t + e_ + 3, 2 * t + e_ + 5):
            off = bl.copy()
            off[index] = NOT_FR
            refused(K.KZG_ERR_INVALID_ARG, b"blinder %d is not below r" % index, None, circ, wires, pub, off)
        # the piece-wise quotient: the same two refusals, and columns that are not the wires' leave a remainder
        ch = [K.Scalar(d[k]) for k in ("alpha", "beta", "gamma", "theta")]
        cols = lambda m=d["m"], b=bl, cc=circ, w=wires: cc.lookup_quotient_blinded(w, GO.to_limbs(d["z"]), GO.to_limbs(m), GO.to_limbs(d["phi"]),
                                                                                  *ch, b, public_inputs=_pi(lcirc), n=n, want_commitments=False)
        assert np.array_equal(cols()[0], GO.to_limbs(d["T"]))
        off = bl.copy()
        off[-1] = NOT_FR
        m2 = list(d["m"])
        m2[2] = (m2[2] + 1) % R
        for call, status, message in ((lambda: cols(b=off), K.KZG_ERR_INVALID_ARG, b"is not below r"),
                                      (lambda: cols(cc=plain), K.KZG_ERR_INVALID_ARG, b"without a lookup table"),
                                      (lambda: cols(m=m2), K.KZG_ERR_REMAINDER, b"not divisible")):
            with pytest.raises(K.KzgError) as ei:
                call()
            assert ei.value.status == status and message in e._lib.kzg_last_error(e._h), e._lib.kzg_last_error(e._h)
        assert np.array_equal(cols()[0], GO.to_limbs(d["T"]))
        # the SRS: none; one point short of n + t + 3; exactly n + t + 3
        bare = K.Engine(0)
        try:
            nokey = _create(bare, lc, log_ext, want_key=False)
            nokey.key = circ.key
            rc, out, _ = _raw(bare, nokey, wires, pub, bl)
            assert rc == K.KZG_ERR_NO_SRS and (out == FILL).all()
            nokey.close()
        finally:
            bare.close()
        for points, status in ((n + t + 2, K.KZG_ERR_DEGREE_TOO_HIGH), (n + t + 3, K.KZG_OK)):
            short = engines.bench_srs(points)
            nokey = _create(short, lc, log_ext, want_key=False)
            nokey.key = circ.key
            rc, out, _ = _raw(short, nokey, wires, pub, bl)
            assert rc == status and (out.tobytes() == d["proof"] if status == K.KZG_OK else (out == FILL).all()), points
            rc, out, _ = _raw(short, nokey, wires, pub, None, fn="kzg_circuit_lookup_prove")
            assert rc == K.KZG_OK  # (the plain proof needs n points)
            nokey.close()
        good()
    finally:
        for x in (circ, broken, plain, small):
            x.close()


# ---- buffers shared with the other provers ---------------------------------------------------------------------------------------
def test_after_a_larger_plain_proof_and_beside_the_other_provers_on_one_handle(oracle):
    """workspaces and cross-round buffers grown by one call are reused or regrown by the next: a blinded lookup proof at 8 rows, a
    plain proof and a plain lookup proof at 2048, the blinded proof again; and on the same handle the plain lookup proof and the
    blinded proof of kzg_circuit_prove keep their bytes.  Then the one prover body under every kind in turn, against the oracles:
    lookup blinded (16, 3, c = 2, 2), plain blinded (8, 3, 2), custom (1, 2, 2), next-row (2, 2, 2), plain (16, 2, 2), lookup
    (8, 3, c = 3, 2) -- the buffers' layout narrows, widens and narrows again under the values the call before left"""
    e = K.SetupArtifactsGenerator(BT.BENCH_SECRET_BE).take(2048 + 8)
    try:
        n, t, c, log_ext = 8, 3, 3, 2
        d = _proof(oracle, n, t, c, log_ext)
        lc, bl = d["lc"], GO.to_limbs(d["bl"].flat())
        circ = _create(e, lc, log_ext)
        wires, pub = _limbs(lc.circuit.wires, n + 5), _pub(d)
        base_bl = bl[:2 * t + 3 + (1 << log_ext) - 2]  # section 4.24's array is the prefix
        old_lookup, old_blinded = circ.lookup_prove(wires, pub, n=n), circ.prove(wires, pub, base_bl, n=n)
        assert circ.lookup_prove_blinded(wires, bl, pub, n=n) == d["proof"]
        big_lc = CC.case(2048, 3, 2, 2).lc
        big = _create(e, big_lc, 2)
        big_wires, big_pub = _limbs(big_lc.circuit.wires), _pi(big_lc.circuit)
        assert len(big.prove(big_wires, big_pub, None)) == K.circuit_proof_size(3, 2)
        assert circ.lookup_prove_blinded(wires, bl, pub, n=n) == d["proof"]
        big_proof = big.lookup_prove_blinded(big_wires, K.circuit_lookup_blinders(3, 2), big_pub)
        assert _verified(oracle, big, big_lc, 2, [] if big_lc.circuit.pi is None else big_lc.circuit.pi, big_proof)
        assert circ.lookup_prove_blinded(wires, bl, pub, n=n) == d["proof"]
        assert circ.lookup_prove(wires, pub, n=n) == old_lookup and circ.prove(wires, pub, base_bl, n=n) == old_blinded
        assert old_lookup != d["proof"]
        # one proof of every kind in turn on this context, nothing recreated in between, each held to its oracle's bytes: every
        # call finds the cross-round buffers at another kind's size and layout, with that kind's values still in them
        d1 = _proof(oracle, 16, 3, 2, 2)
        (bl2, d2), (_, d5) = HC._case(oracle, 8, 3, 2, True, True), HC._case(oracle, 16, 2, 2, True, False)
        d3, d4 = XG._proof(oracle, XC.SHAPES[0]), NG._proof(oracle, NC.SHAPES[0])
        want6 = CC.memo(("bench plain proof of the blinded case", n, t, c, log_ext), lambda: CL.prove(oracle, lc, log_ext, S)["proof"])
        c1, c2, c5 = _create(e, d1["lc"], 2), HC._create(e, d2["c"], 2), HC._create(e, d5["c"], 2)
        c3, c4 = XG._create(e, d3["cc"], XC.SHAPES[0][2], want_key=True), NG._create(e, d4["nc"], NC.SHAPES[0][2], want_key=True)
        steps = [
            ("lookup, blinded, (16, 3, c = 2, 2)",
             lambda: c1.lookup_prove_blinded(_limbs(d1["lc"].circuit.wires), GO.to_limbs(d1["bl"].flat()), _pub(d1)), d1["proof"]),
            ("plain, blinded, (8, 3, 2)", lambda: c2.prove(_limbs(d2["c"].wires), _pub(d2), GO.to_limbs(bl2.flat())), d2["proof"]),
            ("custom, its smallest shape", lambda: c3.custom_prove(_limbs(d3["cc"].circuit.wires), _pub(d3)), d3["proof"]),
            ("next-row, its smallest shape", lambda: c4.custom_next_prove(_limbs(d4["nc"].circuit.wires), _pub(d4)), d4["proof"]),
            ("plain, (16, 2, 2)", lambda: c5.prove(_limbs(d5["c"].wires), _pub(d5), None), d5["proof"]),
            ("lookup, (8, 3, c = 3, 2)", lambda: circ.lookup_prove(wires, pub, n=n), want6),
        ]
        for name, prove, want in steps:
            assert prove() == want, name
        assert want6 == old_lookup
        for handle in (c1, c2, c3, c4, c5):
            handle.close()
        big.close()
        circ.close()
    finally:
        e.close()


def test_on_a_replicated_two_device_context(oracle):
    n, t, c, log_ext = 8, 3, 3, 2
    d = _proof(oracle, n, t, c, log_ext)
    lc, bl = d["lc"], GO.to_limbs(d["bl"].flat())
    wires, pub = _limbs(lc.circuit.wires), _pub(d)
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(BT.BENCH_SECRET_BE, n + t + 3)
        circ = _create(rep, lc, log_ext)
        assert circ.lookup_prove_blinded(wires, bl, pub) == d["proof"]  # forwarded to the circuit's device
        ch = [K.Scalar(d[k]) for k in ("alpha", "beta", "gamma", "theta")]
        coeffs, points = circ.lookup_quotient_blinded(wires, GO.to_limbs(d["z"]), GO.to_limbs(d["m"]), GO.to_limbs(d["phi"]), *ch, bl,
                                                      public_inputs=_pi(lc.circuit))
        assert np.array_equal(coeffs, GO.to_limbs(d["T"])) and len(points) == (1 << log_ext) - 1
        with pytest.raises(K.KzgError) as ei:
            circ.lookup_prove_blinded_device(1 << 20, bl, pub)  # single-device only
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        circ.close()
    finally:
        rep.close()
