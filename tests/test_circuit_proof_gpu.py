"""GPU: proof bytes made by chaining the existing entry points round by round under the hashed transcript
equal the bytes of tests/transcript_oracle.py, and kzg_circuit_verify_proof accepts them.

Every challenge is taken from kzg_circuit_proof_challenges on the bytes written so far (the fields not yet known are zero: a
challenge depends on nothing after it), then handed to the next call: kzg_commit_evaluations_blinded (wires with two blinders, z
with three), kzg_circuit_quotient_blinded, kzg_circuit_open_blinded; the plain chain is kzg_commit_evaluations,
kzg_circuit_quotient, kzg_circuit_open; z comes from kzg_permutation_product.  Shapes (n, t, log_ext): blinded (8, 3, 2),
(256, 3, 2), one tile (2048, 3, 2), two passes (4096, 2, 2) and 31 columns (64, 7, 3); plain one and two rows, (16, 2, 2) and
(4096, 2, 2), whose last chunk is the point at infinity.  Wire stride n + 5."""
import numpy as np
import pytest

import bigint_twin as BT
import blind_oracle as BO
import circuit_oracle as CO
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import perm_quotient_oracle as PQ
import transcript_oracle as TR

pytestmark = pytest.mark.gpu
R = PQ.R
S = BT.fr_from_be_bytes(BT.BENCH_SECRET_BE)
SRS = 4096 + 16
_CACHE = {}  # references computed once, shared and left unchanged


def _case(oracle, n, t, log_ext, with_pi, blinded, seed=0):
    key = (n, t, log_ext, with_pi, blinded, seed)
    if key not in _CACHE:
        c = CO.satisfied(NO.log2_exact(n), t, 900 + n + t, with_pi)
        bl = BO.Blinders.random(t, log_ext, 10 * seed + n + t) if blinded else BO.Blinders.zero(t, log_ext)
        _CACHE[key] = (bl, TR.prove(oracle, c, log_ext, bl, S))
    return _CACHE[key]


def _limbs(cols, stride):
    n = len(cols[0])
    out = np.empty((len(cols), stride, 4), dtype=np.uint64)
    for j, col in enumerate(cols):
        out[j] = GO.to_limbs(list(col) + [0xBAD + i for i in range(stride - n)])
    return out


def _setup(oracle):
    if "setup" not in _CACHE:
        _CACHE["setup"] = (np.stack([oracle.p1_generator()]), np.stack([K.srs_g2_at(BT.BENCH_SECRET_BE, j) for j in range(3)]))
    return _CACHE["setup"]


def _chain(e, circ, c, log_ext, bl, d, blinded):
    """the proof bytes from the existing calls, every challenge from the bytes before it"""
    n, t = c.n, c.t
    L = TR.layout(t, log_ext)
    shifts, public = [K.Scalar(k) for k in c.ks], [K.Scalar(p) for p in d["public"]]
    pi = None if c.pi is None else GO.to_limbs(c.pi)
    proof = bytearray(TR.proof_size(t, log_ext))
    derive = lambda: K.circuit_proof_challenges(circ.key, n, log_ext, shifts, public, bytes(proof))
    put = lambda name, data: proof.__setitem__(slice(*L[name]), data)
    wires, b = _limbs(c.wires, n + 5), GO.to_limbs(bl.flat())
    # round 1
    if blinded:
        wire_points = e.commit_evaluations_blinded(wires, b[:2 * t].reshape(t, 2, 4), n=n)
    else:
        wire_points = [e.commit_evaluations_limbs(GO.to_limbs(col)) for col in c.wires]
    put("wires", b"".join(p.compress() for p in wire_points))
    beta, gamma = derive()[:2]
    # round 2
    zz, last = e.permutation_product_limbs(wires, _limbs(c.sigmas, n + 5), shifts, beta, gamma, n=n)
    assert K.Scalar.from_limbs(last).v == 1 and np.array_equal(zz, GO.to_limbs(d["z"]))
    if blinded:
        z_point = e.commit_evaluations_blinded(zz.reshape(1, n, 4), b[2 * t:2 * t + 3].reshape(1, 3, 4))[0]
    else:
        z_point = e.commit_evaluations_limbs(zz)
    put("z", z_point.compress())
    alpha = derive()[2]
    # round 3
    if blinded:
        tc, t_points = circ.quotient_blinded(wires, zz, alpha, beta, gamma, b, public_inputs=pi)
    else:
        tc, t_points = circ.quotient(wires, zz, alpha, beta, gamma, public_inputs=pi)
    put("chunks", b"".join(p.compress() for p in t_points))
    zeta = derive()[3]
    # round 4: the evaluations are fixed before v.  Chained by hand that takes the evaluation pass twice -- the opening under a
    # placeholder v for the values, then again under the transcript's v for the proof; kzg_circuit_prove forms v in between
    open_ = (lambda v: circ.open_blinded(wires, zz, tc, alpha, beta, gamma, zeta, v, b, public_inputs=pi)) if blinded else \
            (lambda v: circ.open(wires, zz, tc, alpha, beta, gamma, zeta, v, public_inputs=pi))
    (abar, sbar, zw), _ = open_(K.Scalar(1))
    put("evals", b"".join(TR.fr_bytes(x.v) for x in list(abar) + list(sbar) + [zw]))
    v = derive()[4]
    # round 5
    evals2, w_point = open_(v)
    assert [x.v for x in evals2[0]] == [x.v for x in abar] and evals2[2].v == zw.v
    put("w", w_point.compress())
    assert tuple(x.v for x in derive()) == (beta.v, gamma.v, alpha.v, zeta.v, v.v)
    return bytes(proof)


def _create(e, c, log_ext):
    return e.circuit_create(_limbs(c.q_lin, c.n + 3), GO.to_limbs(c.q_mul), GO.to_limbs(c.q_const), _limbs(c.sigmas, c.n + 3),
                            [K.Scalar(k) for k in c.ks], log_ext, n=c.n, want_key=True)


CASES = [(8, 3, 2, True, True), (8, 3, 2, False, True), (256, 3, 2, True, True), (256, 3, 2, False, True), (2048, 3, 2, True, True),
         (4096, 2, 2, True, True), (64, 7, 3, True, True),
         (1, 3, 2, True, False), (2, 3, 2, True, False), (16, 2, 2, True, False), (4096, 2, 2, True, False)]


@pytest.mark.parametrize("n,t,log_ext,with_pi,blinded", CASES)
def test_the_hand_chain_gives_the_oracles_bytes_and_verifies(engines, oracle, n, t, log_ext, with_pi, blinded):
    e = engines.bench_srs(SRS)
    bl, d = _case(oracle, n, t, log_ext, with_pi, blinded)
    c = d["c"]
    circ = _create(e, c, log_ext)
    try:
        assert [p.compress() for p in circ.key] == d["key48"]
        proof = _chain(e, circ, c, log_ext, bl, d, blinded)
        assert proof == d["proof"], [name for name, f in TR.split(proof, t, log_ext).items() if f != TR.split(d["proof"], t, log_ext)[name]]
        g1, g2 = _setup(oracle)
        shifts, public = [K.Scalar(k) for k in c.ks], [K.Scalar(p) for p in d["public"]]
        assert K.circuit_verify_proof(circ.key, n, log_ext, shifts, public, proof, g1, g2)
        bad = bytearray(proof)
        bad[TR.layout(t, log_ext)["evals"][1] - 1] ^= 1
        assert not K.circuit_verify_proof(circ.key, n, log_ext, shifts, public, bytes(bad), g1, g2)
        if public:
            other = [K.Scalar(public[0].v + 1)] + public[1:]
            assert not K.circuit_verify_proof(circ.key, n, log_ext, shifts, other, proof, g1, g2)
    finally:
        circ.close()


def test_two_blinder_sets_give_different_bytes_and_both_verify(engines, oracle):
    n, t, log_ext = 256, 3, 2
    e = engines.bench_srs(SRS)
    (bl0, d0), (bl1, d1) = _case(oracle, n, t, log_ext, True, True), _case(oracle, n, t, log_ext, True, True, seed=1)
    c = d0["c"]
    circ = _create(e, c, log_ext)
    try:
        g1, g2 = _setup(oracle)
        shifts, public = [K.Scalar(k) for k in c.ks], [K.Scalar(p) for p in d0["public"]]
        p1 = _chain(e, circ, c, log_ext, bl1, d1, True)
        assert p1 == d1["proof"] and p1 != d0["proof"]
        f0, f1 = TR.split(d0["proof"], t, log_ext), TR.split(p1, t, log_ext)
        assert all(f0[name] != f1[name] for name in TR.FIELDS)
        assert K.circuit_verify_proof(circ.key, n, log_ext, shifts, public, p1, g1, g2)
        assert K.circuit_verify_proof(circ.key, n, log_ext, shifts, public, d0["proof"], g1, g2)
        # one proof's opening under the other's commitments
        assert not K.circuit_verify_proof(circ.key, n, log_ext, shifts, public, p1[:-48] + d0["proof"][-48:], g1, g2)
    finally:
        circ.close()
