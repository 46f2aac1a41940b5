"""GPU: kzg_circuit_prove / kzg_circuit_prove_device.  The proof bytes equal the bytes of
tests/transcript_oracle.py and the bytes of the existing entry points chained by hand under the same transcript
(tests/test_circuit_proof_gpu.py's chain), and kzg_circuit_verify_proof accepts them.

Shapes (n, t, log_ext): blinded (8, 3, 2), (256, 3, 2), one tile (2048, 3, 2), two passes (4096, 2, 2), 31 columns (64, 7, 3);
plain (1, 3, 2), (2, 3, 2), (4096, 2, 2); with and without public inputs at (8, 3, 2) and (256, 3, 2); wire stride n + 5.  Then two
blinder sets, the statuses with out_proof untouched and the context serving, the slot given back once, the device form inside guard bands, a call after a
larger opening on the same context (regrown workspaces), and two-device contexts."""
import ctypes as C
import threading

import numpy as np
import pytest

import bigint_twin as BT
import blind_oracle as BO
import device_arena as DA
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import test_circuit_proof_gpu as HC  # the oracle cases (shared, computed once) and the hand chain
import transcript_oracle as TR

pytestmark = pytest.mark.gpu
R = HC.R
SRS = HC.SRS
FILL = 0x5A
BLINDED = [(8, 3, 2, True), (8, 3, 2, False), (256, 3, 2, True), (256, 3, 2, False), (2048, 3, 2, True), (4096, 2, 2, True), (64, 7, 3, True)]
PLAIN = [(1, 3, 2, True), (2, 3, 2, True), (4096, 2, 2, True), (8, 3, 2, False)]


def _pub(d):
    return GO.to_limbs(d["public"]) if d["public"] else None


def _bl(bl, blinded):
    return GO.to_limbs(bl.flat()) if blinded else None


def _raw(e, circ, wires, pub, bl, n_public=None, fn="kzg_circuit_prove", stride=None):
    """the C call on a pre-filled output: (status, the output bytes)"""
    rows = np.ascontiguousarray(np.stack([p.p1 for p in circ.key]), dtype=np.uint64)
    out = np.full(K.circuit_proof_size(circ.t, circ.log_ext), FILL, dtype=np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    w = np.ascontiguousarray(wires)
    rc = getattr(e._lib, fn)(e._h, circ._c, ptr(rows), ptr(w), w.shape[1] if stride is None else stride, ptr(pub),
                             (0 if pub is None else pub.shape[0]) if n_public is None else n_public, ptr(bl), ptr(out))
    return rc, out


@pytest.mark.parametrize("n,t,log_ext,with_pi,blinded", [s + (True,) for s in BLINDED] + [s + (False,) for s in PLAIN])
def test_proof_bytes_against_the_oracle_and_the_hand_chain(engines, oracle, n, t, log_ext, with_pi, blinded):
    e = engines.bench_srs(SRS)
    bl, d = HC._case(oracle, n, t, log_ext, with_pi, blinded)
    c = d["c"]
    circ = HC._create(e, c, log_ext)
    try:
        proof = circ.prove(HC._limbs(c.wires, n + 5), _pub(d), _bl(bl, blinded), n=n)
        want = d["proof"]
        assert proof == want, [name for name, f in TR.split(proof, t, log_ext).items() if f != TR.split(want, t, log_ext)[name]]
        assert proof == HC._chain(e, circ, c, log_ext, bl, d, blinded)
        g1, g2 = HC._setup(oracle)
        assert K.circuit_verify_proof(circ.key, n, log_ext, [K.Scalar(k) for k in c.ks], [K.Scalar(p) for p in d["public"]], proof, g1, g2)
        assert circ.prove(HC._limbs(c.wires, n), _pub(d), _bl(bl, blinded)) == want  # packed wires, a second call
    finally:
        circ.close()


def test_two_blinder_sets_on_one_witness(engines, oracle):
    n, t, log_ext = 256, 3, 2
    e = engines.bench_srs(SRS)
    (bl0, d0), (bl1, d1) = HC._case(oracle, n, t, log_ext, True, True), HC._case(oracle, n, t, log_ext, True, True, seed=1)
    c = d0["c"]
    circ = HC._create(e, c, log_ext)
    try:
        wires = HC._limbs(c.wires, n + 5)
        p0, p1 = circ.prove(wires, _pub(d0), _bl(bl0, True), n=n), circ.prove(wires, _pub(d0), _bl(bl1, True), n=n)
        assert p0 == d0["proof"] and p1 == d1["proof"] and p0 != p1
        g1, g2 = HC._setup(oracle)
        shifts, public = [K.Scalar(k) for k in c.ks], [K.Scalar(p) for p in d0["public"]]
        assert K.circuit_verify_proof(circ.key, n, log_ext, shifts, public, p0, g1, g2)
        assert K.circuit_verify_proof(circ.key, n, log_ext, shifts, public, p1, g1, g2)
        fresh = circ.prove(wires, _pub(d0), circ.blinders(), n=n)  # the library's own randomness
        assert fresh not in (p0, p1) and K.circuit_verify_proof(circ.key, n, log_ext, shifts, public, fresh, g1, g2)
    finally:
        circ.close()


def test_statuses_leave_the_output_untouched_and_the_context_serving(engines, oracle):
    n, t, log_ext = 256, 3, 2
    e = engines.bench_srs(SRS)
    bl, d = HC._case(oracle, n, t, log_ext, True, True)
    c = d["c"]
    wires, pub, b = HC._limbs(c.wires, n + 5), _pub(d), _bl(bl, True)
    circ = HC._create(e, c, log_ext)
    # the same circuit with one row's constant changed: the gate fails there, the copy constraints hold
    q_const = list(c.q_const)
    q_const[3] = (q_const[3] + 1) % R
    broken = e.circuit_create(HC._limbs(c.q_lin, n), GO.to_limbs(c.q_mul), GO.to_limbs(q_const), HC._limbs(c.sigmas, n),
                              [K.Scalar(k) for k in c.ks], log_ext, n=n, want_key=True)
    try:
        def good():
            rc, out = _raw(e, circ, wires, pub, b)
            assert rc == 0 and out.tobytes() == d["proof"]

        def refused(status, message, *args, **kw):
            rc, out = _raw(e, *args, **kw)
            assert rc == status and (out == FILL).all(), (rc, message)
            if message:
                assert message in e._lib.kzg_last_error(e._h), e._lib.kzg_last_error(e._h)
            good()

        good()
        for blinders in (b, None):
            refused(K.KZG_ERR_REMAINDER, b"not divisible", broken, wires, pub, blinders)  # an unsatisfied gate row
            moved = wires.copy()  # a broken copy constraint: z does not return to one
            moved[0, 5] = GO.to_limbs([(c.wires[0][5] + 1) % R])[0]
            refused(K.KZG_ERR_REMAINDER, b"z_n != 1", circ, moved, pub, blinders)
        # argument errors, in the header's order
        not_fr = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
        refused(K.KZG_ERR_INVALID_ARG, None, circ, wires, pub, b, stride=n - 1)
        refused(K.KZG_ERR_INVALID_ARG, None, circ, wires, np.concatenate([pub, pub[:1]]), b)  # n_public = n + 1
        bad_pub, bad_b = pub.copy(), b.copy()
        bad_pub[n - 1] = not_fr
        bad_b[2 * t + 1] = not_fr
        refused(K.KZG_ERR_INVALID_ARG, b"public input is not below r", circ, wires, bad_pub, b)
        refused(K.KZG_ERR_INVALID_ARG, b"is not below r", circ, wires, pub, bad_b)
        other = engines.bench_srs(n + t + 3)
        rc, out = _raw(other, circ, wires, pub, b)  # a circuit of another context
        assert rc == K.KZG_ERR_INVALID_ARG and (out == FILL).all()
        good()
    finally:
        circ.close()
        broken.close()


def test_a_proof_gives_back_one_slot_once(engines, oracle):
    """The rounds of a proof run on the call's slot and give nothing back themselves; the call gives it back once.  Seen from
    outside: after a proof, with every slot then taken by a submitted job, a synchronous call finds no slot that another
    synchronous caller could free and is refused with KZG_ERR_BUSY at once.  Were the count of owned slots off after the proof, it
    would wait for one instead: so the call runs on a thread of its own, and if it has not come back the jobs are collected, which
    frees it, before its status is judged."""
    n, t, log_ext = 8, 3, 2
    e = engines.bench_srs(SRS)
    bl, d = HC._case(oracle, n, t, log_ext, True, True)
    c = d["c"]
    circ = HC._create(e, c, log_ext)
    coeffs = GO.to_limbs(list(range(1, n + 1)))
    dptr = e.dev_alloc(coeffs.nbytes)
    status = []

    def synchronous_call():
        try:
            e.commit_limbs(coeffs)
            status.append(0)
        except K.KzgError as err:
            status.append(err.status)

    try:
        assert circ.prove(HC._limbs(c.wires, n), _pub(d), _bl(bl, True)) == d["proof"]
        e.dev_upload(dptr, coeffs)
        slots = e.num_slots()
        for s in range(slots):
            e.commit_submit(s, dptr, n)
        caller = threading.Thread(target=synchronous_call, daemon=True)
        caller.start()
        caller.join(5)
        came_back = not caller.is_alive()
        points = [e.wait(s).compress() for s in range(slots)]
        caller.join(60)
        assert came_back and status == [K.KZG_ERR_BUSY], (came_back, status)
        assert len(set(points)) == 1 and e.commit_limbs(coeffs).compress() == points[0]  # the context serves
    finally:
        e.dev_free(dptr)
        circ.close()


def test_shape_rule_no_srs_and_short_srs(engines, oracle):
    n, t, log_ext = 256, 3, 2
    bl, d = HC._case(oracle, n, t, log_ext, True, True)
    c = d["c"]
    wires, pub, b = HC._limbs(c.wires, n), _pub(d), _bl(bl, True)
    e = engines.bench_srs(SRS)
    key = HC._create(e, c, log_ext)
    bare = K.Engine(0)  # no SRS
    short = engines.bench_srs(n)  # enough for a plain proof and the key, not for a blinded proof
    try:
        for eng, blinders, status in ((bare, b, K.KZG_ERR_NO_SRS), (bare, None, K.KZG_ERR_NO_SRS), (short, b, K.KZG_ERR_DEGREE_TOO_HIGH)):
            circ = eng.circuit_create(HC._limbs(c.q_lin, n), GO.to_limbs(c.q_mul), GO.to_limbs(c.q_const), HC._limbs(c.sigmas, n),
                                      [K.Scalar(k) for k in c.ks], log_ext, n=n, want_key=False)
            circ.key = key.key
            try:
                rc, out = _raw(eng, circ, wires, pub, blinders)
                assert rc == status and (out == FILL).all(), (rc, status)
                if eng is short:  # the plain proof fits: the context serves
                    _, plain = HC._case(oracle, n, t, log_ext, True, False)
                    assert circ.prove(wires, pub, None) == plain["proof"]
            finally:
                circ.close()
        # the shape rule of the blinded calls: N >= t n + t + 4
        bl4, d4 = HC._case(oracle, 4, 3, 2, True, False)
        c4 = d4["c"]
        circ = HC._create(e, c4, 2)
        try:
            rc, out = _raw(e, circ, HC._limbs(c4.wires, 4), _pub(d4), np.zeros((2 * 3 + 3 + 2, 4), dtype=np.uint64))
            assert rc == K.KZG_ERR_INVALID_ARG and (out == FILL).all() and b"t n + t + 4" in e._lib.kzg_last_error(e._h)
            assert circ.prove(HC._limbs(c4.wires, 4), _pub(d4), None) == d4["proof"]
        finally:
            circ.close()
    finally:
        key.close()
        bare.close()


@pytest.mark.parametrize("n,t,log_ext,blinded", [(8, 3, 2, True), (256, 3, 2, True), (4096, 2, 2, True), (2, 3, 2, False)])
def test_device_form_inside_guard_bands(engines, oracle, n, t, log_ext, blinded):
    e = engines.bench_srs(SRS)
    bl, d = HC._case(oracle, n, t, log_ext, True, blinded)
    c = d["c"]
    circ = HC._create(e, c, log_ext)
    try:
        with DA.Arena(e, seed=n + t) as arena:
            r_w = arena.region(n, t, n + 5, "wires", data=HC._limbs(c.wires, n))
            arena.upload()
            proof = circ.prove_device(r_w.ptr, _pub(d), _bl(bl, blinded), stride=n + 5)
            arena.check_untouched()
        assert proof == d["proof"]
    finally:
        circ.close()


def test_after_a_larger_opening_on_the_same_context(oracle):
    """workspaces grown by one call are reused or regrown by the next: a proof at 256 rows, an opening at 2048, the proof again"""
    e = K.SetupArtifactsGenerator(BT.BENCH_SECRET_BE).take(2048 + 16)
    try:
        bl, d = HC._case(oracle, 256, 3, 2, True, True)
        c = d["c"]
        circ = HC._create(e, c, 2)
        wires, pub, b = HC._limbs(c.wires, 256 + 5), _pub(d), _bl(bl, True)
        assert circ.prove(wires, pub, b, n=256) == d["proof"]
        blL, dL = HC._case(oracle, 2048, 3, 2, True, True)
        big = HC._create(e, dL["c"], 2)
        HC._chain(e, big, dL["c"], 2, blL, dL, True)  # ends in kzg_circuit_open_blinded at n = 2048
        assert circ.prove(wires, pub, b, n=256) == d["proof"]
        assert big.prove(HC._limbs(dL["c"].wires, 2048), _pub(dL), _bl(blL, True)) == dL["proof"]
        assert circ.prove(wires, pub, b, n=256) == d["proof"]
        big.close()
        circ.close()
    finally:
        e.close()


def test_two_device_contexts(oracle):
    n, t, log_ext = 256, 3, 2
    bl, d = HC._case(oracle, n, t, log_ext, True, True)
    c = d["c"]
    wires, pub, b = HC._limbs(c.wires, n), _pub(d), _bl(bl, True)
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(BT.BENCH_SECRET_BE, n + t + 3)
        circ = HC._create(rep, c, log_ext)
        assert circ.prove(wires, pub, b) == d["proof"]  # forwarded to the circuit's device
        with pytest.raises(K.KzgError) as ei:
            circ.prove_device(1 << 20, pub, b)  # single-device only
        assert ei.value.status == K.KZG_ERR_INVALID_ARG
        circ.close()
    finally:
        rep.close()
    split = K.Engine(devices=[0, 0])
    try:
        split.srs_generate(BT.BENCH_SECRET_BE, n + t + 3)
        circ = split.circuit_create(HC._limbs(c.q_lin, n), GO.to_limbs(c.q_mul), GO.to_limbs(c.q_const), HC._limbs(c.sigmas, n),
                                    [K.Scalar(k) for k in c.ks], log_ext, n=n, want_key=False)
        circ.key = [K.G1Point(oracle.p1_mult(oracle.p1_generator(), s % R)) for s in d["key_s"]]
        with pytest.raises(K.KzgError) as ei:
            circ.prove(wires, pub, b)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG and "range-split" in str(ei.value)
        circ.close()
    finally:
        split.close()
