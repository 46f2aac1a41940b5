"""CPU: circuit proofs whose custom gates read the next row -- tests/circuit_next_oracle.py against
itself, and the host-only calls kzg_circuit_custom_next_proof_size, kzg_circuit_custom_next_proof_challenges and
kzg_circuit_custom_next_verify_proof against it (hashlib, the big-integer oracles, commitments from a known secret: no GPU).

Shapes (n, t, log_ext, p, p'): the four smallest of tests/circuit_next_cases.py and (64, 6, 3, ..), 32 columns at zeta and 7 at
zeta w.  Next-row proofs are plain."""
import ctypes as C
import os

import numpy as np
import pytest

import blind_oracle as BO
import circuit_custom_oracle as CX
import circuit_next_cases as NC
import circuit_next_oracle as CN
import circuit_oracle as CO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import perm_quotient_oracle as PQ
import trapdoor_oracle as TO

R = PQ.R
SECRET = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % R
SHAPES = NC.SMALL + [NC.WIDE]
INV = K.KZG_ERR_INVALID_ARG
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("beta", "gamma", "alpha", "zeta", "v")
_rows = lambda m: "_".join("".join(map(str, r)) for r in m)
ids = lambda s: "n%d_t%d_e%d_%s_next_%s" % (s[0], s[1], 1 << s[2], _rows(s[3]), _rows(s[4]))


def _proof(oracle, shape, with_pi=True):
    n, t, log_ext, exps, exps_next = shape

    def make():
        cs = NC.case(n, t, log_ext, exps, exps_next, with_pi)
        return CN.prove(oracle, cs.nc, log_ext, SECRET)
    return NC.memo(("proof", shape, with_pi), make)


@pytest.fixture(scope="module")
def srs(oracle):
    """[s^j]G1 for j < 2 and [s^j]G2 for j <= 2"""
    g1 = np.stack([oracle.p1_mult(oracle.p1_generator(), pow(SECRET, j, R)) for j in range(2)])
    g2 = np.stack([K.srs_g2_at(TO.secret_be(SECRET), j) for j in range(3)])
    return g1, g2


def _key(oracle, d, key_s=None):
    return [K.G1Point(oracle.p1_mult(oracle.p1_generator(), s % R)) for s in (d["key_s"] if key_s is None else key_s)]


def _scalars(values):
    return [K.Scalar(x) for x in values]


def _challenges(oracle, d, proof=None, key_s=None, exps=None, exps_next=None, public=None):
    nc = d["nc"]
    got = K.circuit_custom_next_proof_challenges(_key(oracle, d, key_s), nc.n, d["log_ext"], nc.exps if exps is None else exps,
                                                 nc.exps_next if exps_next is None else exps_next, _scalars(nc.circuit.ks),
                                                 _scalars(d["public"] if public is None else public),
                                                 d["proof"] if proof is None else proof)
    return tuple(x.v for x in got)


def _verify(oracle, srs, d, proof=None, key_s=None, exps=None, exps_next=None, public=None):
    nc = d["nc"]
    return K.circuit_custom_next_verify_proof(_key(oracle, d, key_s), nc.n, d["log_ext"], nc.exps if exps is None else exps,
                                              nc.exps_next if exps_next is None else exps_next, _scalars(nc.circuit.ks),
                                              _scalars(d["public"] if public is None else public),
                                              d["proof"] if proof is None else proof, srs[0], srs[1])


def _flip(proof, at, bit=1):
    b = bytearray(proof)
    b[at] ^= bit
    return bytes(b)


# ---- the oracle against itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + [(4, 3, 2, ((1, 1, 0),), ((0, 0, 1),)), (16, 2, 2, ((2, 0), (0, 0)), ((0, 1), (1, 1)))], ids=ids)
def test_oracle_division_degrees_and_the_check_at_a_point(shape):
    n, t, log_ext, exps, exps_next = shape
    cs = NC.case(n, t, log_ext, exps, exps_next)
    e, dm = 1 << log_ext, NC.d_max(exps, exps_next)
    T = cs.quotient  # (asserts a zero remainder and the degrees)
    assert len(cs.gprime) <= (dm + 1) * (n - 1) + 1
    assert len(PQ._trim(T)) <= (e - 1) * n
    w = NO.domain_root(NO.log2_exact(n))
    for zeta in (0x1234567, w, pow(w, n - 1, R)):  # off H, in H, and the point whose next row wraps
        assert CN.check_at(zeta, T, cs.nc, cs.coefs, NC.ALPHA, NC.BETA, NC.GAMMA)
    zeta = 0xFEDCBA987654321
    r = CN.linearisation(cs.nc, cs.coefs, T, log_ext, NC.ALPHA, NC.BETA, NC.GAMMA, zeta)
    assert not any(r[n:]) and PQ.horner(r, zeta) == 0
    # G' on H is the rows' value: the coefficients agree with the row-by-row definition, the wrap included
    assert NO.ntt((cs.gprime + [0] * (8 * n))[:n]) == CN.gprime_rows(cs.nc) if len(cs.gprime) <= n else True
    on_h = [PQ.horner(cs.gprime, pow(w, i, R)) for i in (0, n - 1)]
    rows = CN.gprime_rows(cs.nc)
    assert on_h == [rows[0], rows[n - 1]]


@pytest.mark.parametrize("shape", [NC.NEXT_ONLY, NC.WIDE], ids=ids)
def test_oracle_refuses_a_change_of_one_value(shape):
    n, t, log_ext, exps, exps_next = shape
    cs = NC.case(n, t, log_ext, exps, exps_next)
    nc = cs.nc
    zeta = 0xFEDCBA987654321
    s = next(s for s in range(nc.g) if any(nc.exps_next[s]))
    assert nc.q_custom[s][n - 1]  # the term of row n - 1 reads row 0
    j = next(j for j in range(t) if nc.exps_next[s][j])
    wires = [list(col) for col in nc.circuit.wires]
    wires[j][0] = (wires[j][0] + 1) % R  # row 0 as the NEXT row of row n - 1 (and, where wire j is read there, as row 0 itself)
    qx = [list(col) for col in nc.q_custom]
    qx[s][n - 1] = (qx[s][n - 1] + 1) % R
    s0 = next(s for s in range(nc.g) if any(nc.exps[s]))
    j0 = next(j for j in range(t) if nc.exps[s0][j])
    ex = [list(r) for r in nc.exps]
    ex[s0][j0] -= 1
    en = [list(r) for r in nc.exps_next]
    en[s][j] += 1 if sum(en[s]) + sum(nc.exps[s]) < nc.d_max or nc.d_max < (1 << log_ext) - 1 else -1
    assert CN.remainder(nc, cs.z, NC.ALPHA, NC.BETA, NC.GAMMA) == []
    for kw in (dict(wires=wires), dict(q_custom=qx), dict(exps=ex), dict(exps_next=en)):
        assert CN.remainder(nc, cs.z, NC.ALPHA, NC.BETA, NC.GAMMA, **kw) != [], sorted(kw)
    # and with the true quotient, r_N formed from a changed wire value, selector value, exponent or next-row exponent does not
    # vanish at zeta
    T = cs.quotient
    key, wc, zc, pi = cs.coefs
    wc2 = [NO.intt(col) + [0, 0] for col in wires]
    key2 = key[:2 * t + 2] + [NO.intt(col) for col in qx]
    for coefs, kw in (((key, wc2, zc, pi), {}), ((key2, wc, zc, pi), {}), (cs.coefs, dict(exps=ex)), (cs.coefs, dict(exps_next=en))):
        r = CN.linearisation(nc, coefs, T, log_ext, NC.ALPHA, NC.BETA, NC.GAMMA, zeta, **kw)
        assert PQ.horner(r, zeta) != 0, sorted(kw)
    assert PQ.horner(CN.linearisation(nc, cs.coefs, T, log_ext, NC.ALPHA, NC.BETA, NC.GAMMA, zeta), zeta) == 0


# ---- exports and sizes -------------------------------------------------------------------------------------------------------------
def test_exports():
    lib = K.load_library()
    header = open(os.path.join(HERE, "..", "include", "kzg_mi355x.h")).read()
    for name in ("kzg_circuit_create_custom_next", "kzg_circuit_custom_next_gate", "kzg_circuit_custom_next_quotient",
                 "kzg_circuit_custom_next_prove", "kzg_circuit_custom_next_prove_device", "kzg_circuit_custom_next_proof_size",
                 "kzg_circuit_custom_next_proof_challenges", "kzg_circuit_custom_next_verify_proof"):
        assert name in K.ABI_SYMBOLS and hasattr(lib, name) and ("int %s(" % name) in header, name
    assert K.KZG_ABI_VERSION == 4 == lib.kzg_abi_version()
    assert CN.DST.decode() in header and len(CN.DST) == 31
    hpp = open(os.path.join(HERE, "..", "include", "kzg_mi355x.hpp")).read()
    assert "custom_next" not in hpp  # the C++ header is not extended


def test_proof_sizes():
    lib = K.load_library()
    for t in range(1, 9):
        for log_ext in range(0, 5):
            for rho in range(0, 9):
                legal = 2 <= t <= K.KZG_PQ_MAX_COLUMNS and log_ext <= K.KZG_PQ_MAX_LOG_EXT and t + 1 <= (1 << log_ext) and 1 <= rho <= t
                out = C.c_size_t(123)
                rc = lib.kzg_circuit_custom_next_proof_size(t, log_ext, rho, C.byref(out))
                if legal:
                    assert rc == 0 and out.value == CN.proof_size(t, log_ext, rho) == K.circuit_proof_size(t, log_ext) + 32 * rho
                else:
                    assert rc == INV and out.value == 123, (t, log_ext, rho)
    assert lib.kzg_circuit_custom_next_proof_size(3, 2, 1, None) == INV
    assert K.circuit_custom_next_proof_size(3, 2, 2) == 48 * 8 + 32 * 8


# ---- the transcript --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_challenges_against_the_oracle(oracle, shape):
    d = _proof(oracle, shape)
    want = tuple(d[k] for k in NAMES)
    assert _challenges(oracle, d) == want and len(set(want)) == 5
    if shape == NC.NEXT_ONLY:
        d0 = _proof(oracle, shape, with_pi=False)
        assert d0["public"] == [] and _challenges(oracle, d0) == tuple(d0[k] for k in NAMES)


@pytest.mark.parametrize("shape", [NC.NEXT_ONLY, (16, 2, 2, ((1, 0),), ((0, 1),))], ids=ids)
def test_challenges_with_no_one_and_n_public_inputs(oracle, shape):
    """the two ends of the statement's public inputs and one value, at (8, 3, 2) with e = t + 1 and at (16, 2, 2) with e > t + 1.
    The proof's bytes are hashed as they are: the same proof serves every statement"""
    n, t, log_ext, exps, exps_next = shape
    d = _proof(oracle, shape)
    nc = d["nc"]
    assert len(d["public"]) == n
    seen = set()
    for n_public in (0, 1, n):
        public = d["public"][:n_public]
        got = _challenges(oracle, d, public=public)
        assert got == CN.challenges(n, t, log_ext, nc.exps, nc.exps_next, nc.circuit.ks, d["key48"], public, d["proof"]), n_public
        seen.add(got)
    assert len(seen) == 3 and tuple(d[k] for k in NAMES) in seen


def test_every_field_of_the_statement_moves_every_challenge(oracle):
    n, t, log_ext, exps, exps_next = NC.NEXT_ONLY
    d = _proof(oracle, NC.NEXT_ONLY)
    nc, base = d["nc"], _challenges(oracle, d)
    moved = lambda got: all(a != b for a, b in zip(got, base))
    # g: one term more (the key one commitment longer), with the same R so that the proof's length stays
    assert moved(_challenges(oracle, d, key_s=d["key_s"] + d["key_s"][-1:], exps=nc.exps + [[1, 0, 0]], exps_next=nc.exps_next + [[0, 1, 0]]))
    ex = [list(r) for r in nc.exps]
    ex[0][2] += 1
    assert moved(_challenges(oracle, d, exps=ex))
    for s in range(nc.g):  # each byte of p', R kept: 0 -> 1 only where the wire's column already has an entry, else 1 -> 2 ..
        for j in range(t):
            en = [list(r) for r in nc.exps_next]
            en[s][j] += 1
            if CN.next_wires(en) != nc.R or not CN.shape_ok(n, t, log_ext, nc.exps, en):
                continue
            assert moved(_challenges(oracle, d, exps_next=en)), (s, j)
    seen = 0
    for at in range(nc.g * t):  # ... and every byte against the oracle's hash directly, whatever it does to R
        en = [list(r) for r in nc.exps_next]
        en[at // t][at % t] ^= 1
        h0 = CN.statement_hash(n, t, log_ext, nc.exps, en, nc.circuit.ks, d["key48"], d["public"])
        assert h0 != CN.statement_hash(n, t, log_ext, nc.exps, nc.exps_next, nc.circuit.ks, d["key48"], d["public"])
        if CN.shape_ok(n, t, log_ext, nc.exps, en) and len(CN.next_wires(en)) == nc.rho:
            want = CN.challenges(n, t, log_ext, nc.exps, en, nc.circuit.ks, d["key48"], d["public"], d["proof"])
            assert _challenges(oracle, d, exps_next=en) == want and moved(want)
            seen += 1
    assert seen >= 1
    # p and p' swapped: another statement
    assert CN.statement_hash(n, t, log_ext, nc.exps_next, nc.exps, nc.circuit.ks, d["key48"], d["public"]) != \
        CN.statement_hash(n, t, log_ext, nc.exps, nc.exps_next, nc.circuit.ks, d["key48"], d["public"])
    for j in (0, 2 * t + 2, 2 * t + 3):
        ks = list(d["key_s"])
        ks[j] = (ks[j] + 1) % R
        assert moved(_challenges(oracle, d, key_s=ks))
    pub = list(d["public"])
    pub[-1] = (pub[-1] + 1) % R
    assert moved(_challenges(oracle, d, public=pub))
    # from h1 on the chain is the plain proof's: the fields move what comes after them; v follows ALL 2 t + rho evaluations
    lay = CN.layout(t, log_ext, nc.rho)
    for name, first in {"wires": 0, "z": 2, "chunks": 3, "evals": 4}.items():
        a, b = lay[name]
        got = _challenges(oracle, d, proof=_flip(d["proof"], b - 1))
        assert got[:first] == base[:first] and all(x != y for x, y in zip(got[first:], base[first:])), name
    a, b = lay["evals"]
    for i in range(2 * t + nc.rho):
        got = _challenges(oracle, d, proof=_flip(d["proof"], a + 32 * i + 31))
        assert got[:4] == base[:4] and got[4] != base[4], i


# ---- the verifier ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_verifier_accepts_the_oracles_proofs(oracle, srs, shape):
    n, t, log_ext, exps, exps_next = shape
    d = _proof(oracle, shape)
    assert len(d["proof"]) == K.circuit_custom_next_proof_size(t, log_ext, NC.rho(exps_next))
    assert _verify(oracle, srs, d)
    if shape == NC.NEXT_ONLY:
        assert _verify(oracle, srs, _proof(oracle, shape, with_pi=False))


def test_verifier_rejects_a_change_in_each_field_the_key_and_the_statement(oracle, srs):
    n, t, log_ext, exps, exps_next = NC.NEXT_ONLY
    d = _proof(oracle, NC.NEXT_ONLY)
    nc = d["nc"]
    assert _verify(oracle, srs, d)
    for name, (a, b) in CN.layout(t, log_ext, nc.rho).items():
        if name == "evals":
            for i in range(2 * t + nc.rho):  # the rho new scalars included
                assert not _verify(oracle, srs, d, proof=_flip(d["proof"], a + 32 * i + 31)), (name, i)
        else:
            other = TO.g1_scalar(oracle, 0xABCDEF)
            assert not _verify(oracle, srs, d, proof=d["proof"][:a] + other + d["proof"][a + 48:]), name
    # the two new scalars swapped
    a, b = CN.layout(t, log_ext, nc.rho)["evals"]
    p = d["proof"]
    assert not _verify(oracle, srs, d, proof=p[:b - 64] + p[b - 32:b] + p[b - 64:b - 32] + p[b:])
    ks = list(d["key_s"])
    ks[2 * t + 2], ks[2 * t + 3] = ks[2 * t + 3], ks[2 * t + 2]  # two custom commitments swapped
    assert ks != d["key_s"] and not _verify(oracle, srs, d, key_s=ks)
    # swapped matrices (a legal shape too), swapped rows of p', one exponent moved within p'
    with pytest.raises(K.KzgError):  # (here the swap changes rho, and with it the length a proof must have)
        _verify(oracle, srs, d, exps=nc.exps_next, exps_next=nc.exps)
    db = _proof(oracle, NC.BOTH_ROWS)  # p = [[3,0,0]], p' = [[4,0,0]]: the swap keeps R and the length
    assert _verify(oracle, srs, db) and not _verify(oracle, srs, db, exps=db["nc"].exps_next, exps_next=db["nc"].exps)
    assert not _verify(oracle, srs, d, exps_next=[nc.exps_next[1], nc.exps_next[0]])
    en = [list(r) for r in nc.exps_next]
    en[1][2] -= 1
    assert CN.next_wires(en) == nc.R and not _verify(oracle, srs, d, exps_next=en)
    ex = [list(r) for r in nc.exps]
    ex[0][0], ex[0][2] = ex[0][2], ex[0][0]
    assert not _verify(oracle, srs, d, exps=ex)
    pub = list(d["public"])
    pub[0] = (pub[0] + 1) % R
    assert not _verify(oracle, srs, d, public=pub)
    # a proof of the wrong length is an argument error
    for proof in (d["proof"][:-1], d["proof"] + b"\0", d["proof"][:b - 32] + d["proof"][b:]):
        with pytest.raises(K.KzgError):
            _verify(oracle, srs, d, proof=proof)


def test_a_custom_proof_is_no_next_row_proof_and_the_other_way_round(oracle, srs):
    n, t, log_ext, exps, exps_next = NC.BOTH_ROWS
    d = _proof(oracle, NC.BOTH_ROWS)
    nc = d["nc"]
    shifts, public = _scalars(nc.circuit.ks), _scalars(d["public"])
    key = _key(oracle, d)
    lay = CN.layout(t, log_ext, nc.rho)
    a, b = lay["evals"]
    # the next-row proof under the custom verifier of the same key and p: its own bytes have another length; without the rho
    # scalars the length is a custom proof's and the proof is invalid
    with pytest.raises(K.KzgError):
        K.circuit_custom_verify_proof(key, n, log_ext, nc.exps, shifts, public, d["proof"], *srs)
    cut = d["proof"][:b - 32 * nc.rho] + d["proof"][b:]
    assert len(cut) == K.circuit_proof_size(t, log_ext)
    assert not K.circuit_custom_verify_proof(key, n, log_ext, nc.exps, shifts, public, cut, *srs)
    # the custom statement with the same p does not hold for these wires, so there is no custom proof of this key; a custom proof
    # of the twin circuit (same wires, permutation, selectors and p, q_C satisfying the custom gate) is no next-row proof: neither
    # of its own key nor of this one, with the true values f_j(zeta w) put where the format wants them
    c = nc.circuit
    base = CO.Circuit(c.ks, c.wires, c.sigmas, c.q_lin, c.q_mul, [0] * n, c.pi)
    twin = CX.CustomCircuit(base, nc.q_custom, nc.exps)
    base.q_const = [(-v) % R for v in CX.gate_rows(twin)]
    cp = CX.prove(oracle, twin, log_ext, BO.Blinders.zero(t, log_ext), SECRET)
    twin_key = [K.G1Point(oracle.p1_mult(oracle.p1_generator(), s)) for s in cp["key_s"]]
    assert K.circuit_custom_verify_proof(twin_key, n, log_ext, nc.exps, shifts, public, cp["proof"], *srs)
    w = NO.domain_root(NO.log2_exact(n))
    extra = b"".join(PQ.horner(cp["coefs"][1][j], cp["zeta"] * w % R).to_bytes(32, "big") for j in nc.R)
    grown = cp["proof"][:b - 32 * nc.rho] + extra + cp["proof"][b - 32 * nc.rho:]
    assert len(grown) == len(d["proof"])
    assert not _verify(oracle, srs, d, proof=grown)
    assert not _verify(oracle, srs, d, proof=grown, key_s=cp["key_s"])
    # ... and for every p' over the same p, the custom proof stays a custom proof only
    for en in ([[1, 0, 0]], [[0, 1, 0]], [[0, 0, 2]], [[1, 1, 1]]):
        rho = len(CN.next_wires(en))
        ex2 = b"".join(PQ.horner(cp["coefs"][1][j], cp["zeta"] * w % R).to_bytes(32, "big") for j in CN.next_wires(en))
        g2 = cp["proof"][:b - 32 * nc.rho] + ex2 + cp["proof"][b - 32 * nc.rho:]
        assert len(g2) == CN.proof_size(t, log_ext, rho)
        assert not _verify(oracle, srs, d, proof=g2, key_s=cp["key_s"], exps_next=en), en


def test_undecodable_bytes_are_invalid_not_an_error(oracle, srs):
    n, t, log_ext, exps, exps_next = NC.NEXT_ONLY
    d = _proof(oracle, NC.NEXT_ONLY)
    rho = d["nc"].rho
    lay = CN.layout(t, log_ext, rho)
    for name in ("wires", "z", "chunks", "w"):
        a, _ = lay[name]
        assert not _verify(oracle, srs, d, proof=_flip(d["proof"], a, 0x80)), name  # the compression flag cleared
        assert not _verify(oracle, srs, d, proof=d["proof"][:a] + b"\xff" * 48 + d["proof"][a + 48:]), name
    a, _ = lay["evals"]
    for i in (0, 2 * t - 1, 2 * t, 2 * t + rho - 1):
        assert not _verify(oracle, srs, d, proof=d["proof"][:a + 32 * i] + R.to_bytes(32, "big") + d["proof"][a + 32 * (i + 1):]), i


def test_argument_errors_and_every_shape_rule(oracle, srs):
    n, t, log_ext, exps, exps_next = NC.NEXT_ONLY
    g = len(exps)
    d = _proof(oracle, NC.NEXT_ONLY)
    nc = d["nc"]
    lib = K.load_library()
    rows = np.ascontiguousarray(np.stack([k.p1 for k in _key(oracle, d)]), dtype=np.uint64)
    ks = np.ascontiguousarray(np.stack([K.Scalar(k).limbs() for k in nc.circuit.ks]), dtype=np.uint64)
    pub = np.ascontiguousarray(np.stack([K.Scalar(p).limbs() for p in d["public"]]), dtype=np.uint64)
    buf = np.frombuffer(d["proof"], dtype=np.uint8)
    ex, en = np.array(nc.exps, dtype=np.uint8), np.array(nc.exps_next, dtype=np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    ok = C.c_int(7)

    def verify(rows=rows, n=n, t=t, log_ext=log_ext, g=g, ex=ex, en=en, ks=ks, pub=pub, n_public=len(d["public"]), buf=buf,
               length=len(d["proof"]), g1=srs[0], g2=srs[1], valid=C.byref(ok)):
        return lib.kzg_circuit_custom_next_verify_proof(ptr(rows), n, t, log_ext, g, ptr(ex), ptr(en), ptr(ks), ptr(pub), n_public, ptr(buf),
                                                        length, ptr(g1), 144, ptr(g2), 288, valid)
    assert verify() == 0 and ok.value == 1
    ok.value = 7
    not_fr = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    bad_pub, bad_ks, bad_rows = pub.copy(), ks.copy(), rows.copy()
    bad_pub[1], bad_ks[0] = not_fr, not_fr
    bad_rows[2 * t + 2, 0] ^= 1  # a custom commitment off the curve
    zero_term, big_exp, big_next, deg4, no_next = en.copy(), ex.copy(), en.copy(), en.copy(), np.zeros_like(en)
    zero_term[1] = 0       # the second term has p = 0: without p' its degree is 0
    big_exp[0, 0] = 8      # an exponent above 7
    big_next[1, 2] = 8
    deg4[1] = (0, 2, 2)    # d_max = 4 > e - 1 = 3
    for kw in (dict(rows=None), dict(ex=None), dict(en=None), dict(ks=None), dict(pub=None), dict(buf=None), dict(g1=None), dict(g2=None),
               dict(valid=None), dict(n=6), dict(t=1), dict(t=8), dict(log_ext=4), dict(g=0), dict(g=9), dict(n_public=n + 1),
               dict(length=len(d["proof"]) - 1), dict(length=len(d["proof"]) + 1), dict(length=len(d["proof"]) - 32 * nc.rho),
               dict(pub=bad_pub), dict(ks=bad_ks), dict(rows=bad_rows), dict(en=zero_term), dict(ex=big_exp), dict(en=big_next),
               dict(en=deg4), dict(en=no_next)):
        assert verify(**kw) == INV and ok.value == 7, sorted(kw)
    out = np.zeros((5, 4), dtype=np.uint64)
    args = lambda **kw: [kw.get("rows", ptr(rows)), kw.get("n", n), t, log_ext, kw.get("g", g), kw.get("ex", ptr(ex)), kw.get("en", ptr(en)),
                         ptr(ks), ptr(pub), len(d["public"]), ptr(buf), kw.get("length", len(d["proof"])), kw.get("out", ptr(out))]
    assert lib.kzg_circuit_custom_next_proof_challenges(*args()) == 0
    for kw in (dict(rows=None), dict(ex=None), dict(en=None), dict(out=None), dict(n=6), dict(g=0), dict(g=9), dict(length=3),
               dict(en=ptr(zero_term)), dict(ex=ptr(big_exp)), dict(en=ptr(big_next)), dict(en=ptr(deg4)), dict(en=ptr(no_next))):
        assert lib.kzg_circuit_custom_next_proof_challenges(*args(**kw)) == INV, sorted(kw)
    # every rule by shape: e >= d_max + 1 over both matrices, the column count at zeta, rho = 0, n = 1
    one = np.zeros((5, 4), dtype=np.uint64)
    for nn, tt, le, p, pn, legal in ((8, 3, 2, [[2, 0, 0]], [[0, 1, 0]], True), (8, 3, 2, [[2, 1, 0]], [[0, 1, 0]], False),
                                     (8, 3, 2, [[0, 0, 0]], [[0, 0, 3]], True), (8, 3, 2, [[3, 0, 0]], [[0, 0, 0]], False),
                                     (1, 2, 2, [[1, 0]], [[0, 1]], False), (2, 2, 2, [[1, 0]], [[0, 1]], True),
                                     (8, 6, 3, [[1, 0, 0, 0, 0, 0]] * 3, [[0, 0, 0, 0, 0, 1]] * 3, True),
                                     (8, 6, 3, [[1, 0, 0, 0, 0, 0]] * 4, [[0, 0, 0, 0, 0, 1]] * 4, False),
                                     (8, 2, 1, [[1, 0]], [[0, 1]], False), (8, 2, 2, [[1, 0]] * 8, [[0, 1]] * 8, True),
                                     (8, 3, 3, [[7, 0, 0]], [[0, 1, 0]], False), (8, 3, 3, [[0, 0, 0]], [[7, 0, 0]], True)):
        assert CN.shape_ok(nn, tt, le, p, pn) == legal, (nn, tt, le, p, pn)
        gg = len(p)
        key = np.tile(rows[0], (2 * tt + 2 + gg, 1))
        pb, pnb = np.array(p, dtype=np.uint8), np.array(pn, dtype=np.uint8)
        sh = np.tile(ks[0], (tt, 1))
        rho = len(CN.next_wires(pn))
        proof = np.zeros(CN.proof_size(tt, le, max(rho, 1)) if tt + 1 <= (1 << le) else 64, dtype=np.uint8)
        rc = lib.kzg_circuit_custom_next_proof_challenges(ptr(key), nn, tt, le, gg, ptr(pb), ptr(pnb), ptr(sh), None, 0, ptr(proof), len(proof),
                                                          ptr(one))
        assert (rc == 0) == legal, (nn, tt, le, p, pn, rc)
