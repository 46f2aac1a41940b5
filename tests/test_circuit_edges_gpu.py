"""GPU: kzg_circuit_prove / kzg_circuit_prove_device on the circuits of tests/circuit_edge_cases.py.  The
proof bytes equal the bytes of tests/transcript_oracle.py and of the existing entry points chained by hand with the PI column passed
in full (tests/test_circuit_proof_gpu.py's chain), and kzg_circuit_verify_proof accepts them under the n_public-long statement.

Partial public inputs (0 < n_public < n) take the one path that zeroes the PI column of a buffer the context keeps between calls and
copies n_public values over it; the degenerate circuits put all-zero scalar vectors through the commitments, and the point at
infinity they give through the compression and the transcript.

Shapes (n, t, log_ext), each with wire stride n + 5 and then packed: partial blinded (8, 3, 2) with n_public 1 and 7, (256, 3, 2)
and two passes (4096, 2, 2) with 16, (64, 7, 3) with 2; partial plain (2, 3, 2) with 1 and (256, 3, 2) with 16; zero public inputs
at (8, 3, 2); every degenerate builder at (8, 3, 2) and (256, 3, 2), plain and blinded; the idle circuit with one row.  Then the
key commitments, a partial proof after a full one on the same context (stale rows), the device form inside guard bands, and the
statuses with the output untouched."""
import numpy as np
import pytest

import blind_oracle as BO
import circuit_edge_cases as EC
import device_arena as DA
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import test_circuit_proof_gpu as HC  # _limbs, _create, _chain, _setup, the SRS length and the full-PI oracle cases
import test_circuit_prove_gpu as PG  # _raw, _pub, _bl
import transcript_oracle as TR

pytestmark = pytest.mark.gpu
R = HC.R
SRS = HC.SRS
FILL = PG.FILL
_CACHE = {}  # references computed once, shared and left unchanged


def _case(oracle, name, args, log_ext, blinded):
    key = (name, args, log_ext, blinded)
    if key not in _CACHE:
        c = EC.build(name, *args)
        bl = BO.Blinders.random(c.t, log_ext, 333 + c.n + c.t) if blinded else BO.Blinders.zero(c.t, log_ext)
        _CACHE[key] = (bl, EC.prove(oracle, c, log_ext, bl, HC.S))
    return _CACHE[key]


def _statement(c, d):
    return [K.Scalar(k) for k in c.ks], [K.Scalar(p) for p in d["public"]]


def _differing(proof, want, t, log_ext):
    return [name for name, f in TR.split(proof, t, log_ext).items() if f != TR.split(want, t, log_ext)[name]]


P256 = ("partial_public", (8, 3, 16, 33), 2)
DEGENERATE = [("constant_witness", (k, 3, value, 40 + k), 2) for k in (3, 8) for value in (0, EC.VALUE)] + \
             [("idle", (k, 3), 2) for k in (3, 8)] + [("zero_column", (k, 3, 50 + k), 2) for k in (3, 8)]
CASES = [("partial_public", (3, 3, 1, 31), 2, True), ("partial_public", (3, 3, 7, 32), 2, True), P256 + (True,),
         ("partial_public", (12, 2, 16, 34), 2, True), ("partial_public", (6, 7, 2, 35), 3, True),
         ("partial_public", (1, 3, 1, 36), 2, False), P256 + (False,), ("zero_public", (3, 3, 3), 2, True)] + \
        [case + (blinded,) for case in DEGENERATE for blinded in (False, True)] + [("idle", (0, 3), 2, False)]
_ids = lambda cases: ["%s-%s-%s" % (c[0], "x".join(str(a)[:6] for a in c[1]), "blinded" if c[3] else "plain") for c in cases]


@pytest.mark.parametrize("name,args,log_ext,blinded", CASES, ids=_ids(CASES))
def test_proof_bytes_against_the_oracle_and_the_hand_chain(engines, oracle, name, args, log_ext, blinded):
    e = engines.bench_srs(SRS)
    bl, d = _case(oracle, name, args, log_ext, blinded)
    c, want = d["c"], d["proof"]
    n, t = c.n, c.t
    assert len(d["public"]) == (c.n_public or 0)
    if name in ("partial_public", "zero_public"):
        assert 0 < len(d["public"]) < n
    # the points at infinity the case is about are in the oracle's bytes
    inf = EC.infinities(want, t, log_ext)
    if blinded:
        assert inf == []
    else:
        expected = EC.expected_infinities(name, args, t, log_ext)
        assert expected is None or (expected and set(expected) <= set(inf)), (expected, inf)
    circ = HC._create(e, c, log_ext)
    try:
        assert [p.compress() for p in circ.key] == d["key48"]
        proof = circ.prove(HC._limbs(c.wires, n + 5), PG._pub(d), PG._bl(bl, blinded), n=n)
        assert proof == want, _differing(proof, want, t, log_ext)
        chained = HC._chain(e, circ, c, log_ext, bl, d, blinded)  # the PI column in full: all n rows
        assert proof == chained, _differing(proof, chained, t, log_ext)
        g1, g2 = HC._setup(oracle)
        shifts, public = _statement(c, d)
        assert K.circuit_verify_proof(circ.key, n, log_ext, shifts, public, proof, g1, g2)
        if 0 < len(public) < n:  # the same PI polynomial under a longer statement
            assert not K.circuit_verify_proof(circ.key, n, log_ext, shifts, public + [K.Scalar(0)], proof, g1, g2)
        packed = circ.prove(HC._limbs(c.wires, n), PG._pub(d), PG._bl(bl, blinded))  # a second call
        assert packed == want, _differing(packed, want, t, log_ext)
    finally:
        circ.close()


def test_key_commitments_of_the_degenerate_circuits(engines, oracle):
    """kzg_circuit_create's commitments of all-zero and constant columns, infinities included"""
    e = engines.bench_srs(SRS)
    for name, args, log_ext in DEGENERATE + [("idle", (0, 3), 2)]:
        _, d = _case(oracle, name, args, log_ext, False)
        c = d["c"]
        circ = HC._create(e, c, log_ext)
        try:
            got = [p.compress() for p in circ.key]
            assert got == d["key48"], (name, args, [j for j in range(2 * c.t + 2) if got[j] != d["key48"][j]])
            at_infinity = [j for j, k48 in enumerate(got) if k48 == TR.INFINITY48]
            assert at_infinity == (list(range(c.t + 2)) if name == "idle" else []), (name, args)
        finally:
            circ.close()


def test_a_partial_proof_after_a_full_one_finds_no_stale_rows(engines, oracle):
    """The values buffer lives with the context: after a proof with public inputs on all n rows the PI column still holds them, and
    after a larger proof the PI column of a smaller one lies where wires were"""
    e = engines.bench_srs(SRS)
    blF, dF = HC._case(oracle, 256, 3, 2, True, True)
    assert len(dF["public"]) == 256 and any(dF["public"][16:])
    runs = {"full": (blF, dF, True)}
    for key, (name, args, log_ext), blinded in (("partial", P256, True), ("partial plain", P256, False),
                                                 ("small", ("partial_public", (3, 3, 1, 31), 2), True)):
        runs[key] = _case(oracle, name, args, log_ext, blinded) + (blinded,)
    circs = {key: HC._create(e, d["c"], 2) for key, (bl, d, blinded) in runs.items() if key != "partial plain"}
    circs["partial plain"] = circs["partial"]
    try:
        for key in ("full", "partial", "full", "partial", "full", "partial plain", "full", "small", "partial", "small"):
            bl, d, blinded = runs[key]
            c = d["c"]
            proof = circs[key].prove(HC._limbs(c.wires, c.n), PG._pub(d), PG._bl(bl, blinded))
            assert proof == d["proof"], (key, _differing(proof, d["proof"], c.t, 2))
    finally:
        for key, circ in circs.items():
            if key != "partial plain":
                circ.close()


@pytest.mark.parametrize("name,args,log_ext,blinded", [P256 + (True,), ("constant_witness", (3, 3, 0, 43), 2, False)],
                         ids=["partial", "zero_witness"])
def test_device_form_inside_guard_bands(engines, oracle, name, args, log_ext, blinded):
    e = engines.bench_srs(SRS)
    bl, d = _case(oracle, name, args, log_ext, blinded)
    c = d["c"]
    n, t = c.n, c.t
    circ = HC._create(e, c, log_ext)
    try:
        with DA.Arena(e, seed=n + t) as arena:
            r_w = arena.region(n, t, n + 5, "wires", data=HC._limbs(c.wires, n))
            arena.upload()
            proof = circ.prove_device(r_w.ptr, PG._pub(d), PG._bl(bl, blinded), stride=n + 5)
            arena.check_untouched()
        assert proof == d["proof"], _differing(proof, d["proof"], t, log_ext)
    finally:
        circ.close()


def test_statuses_leave_the_output_untouched_and_the_context_serving(engines, oracle):
    e = engines.bench_srs(SRS)
    not_fr = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)

    def served(circ, wires, d, b):
        rc, out = PG._raw(e, circ, wires, PG._pub(d), b)
        assert rc == 0 and out.tobytes() == d["proof"]

    def refused(status, message, circ, wires, pub, b):
        rc, out = PG._raw(e, circ, wires, pub, b)
        assert rc == status and (out == FILL).all(), (rc, message)
        assert message in e._lib.kzg_last_error(e._h), e._lib.kzg_last_error(e._h)

    # a public input that is no field element, at the last index the statement reads
    bl, d = _case(oracle, *P256, True)
    c = d["c"]
    n_public = len(d["public"])
    wires, b = HC._limbs(c.wires, c.n + 5), PG._bl(bl, True)
    circ = HC._create(e, c, 2)
    try:
        served(circ, wires, d, b)
        bad = PG._pub(d).copy()
        assert bad.shape == (n_public, 4) and n_public == 16
        bad[n_public - 1] = not_fr
        refused(K.KZG_ERR_INVALID_ARG, b"public input is not below r", circ, wires, bad, b)
        served(circ, wires, d, b)
    finally:
        circ.close()
    # a broken copy constraint beside the unused column: one cell that the permutation moves takes another value
    name, args, log_ext = DEGENERATE[-1]
    assert name == "zero_column"
    (bl, d), (_, plain) = _case(oracle, name, args, log_ext, True), _case(oracle, name, args, log_ext, False)
    c = d["c"]
    labels = GO.identity_sigmas(args[0], c.ks)
    j, i = next((j, i) for j in range(c.t - 1) for i in range(c.n) if c.sigmas[j][i] != labels[j][i])
    wires, b = HC._limbs(c.wires, c.n + 5), PG._bl(bl, True)
    moved = wires.copy()
    moved[j, i] = GO.to_limbs([(c.wires[j][i] + 1) % R])[0]
    circ = HC._create(e, c, log_ext)
    try:
        served(circ, wires, d, b)
        for blinders, good in ((b, d), (None, plain)):
            refused(K.KZG_ERR_REMAINDER, b"z_n != 1", circ, moved, PG._pub(d), blinders)
            served(circ, wires, good, blinders)
    finally:
        circ.close()
