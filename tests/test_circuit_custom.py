"""CPU: circuit proofs with custom gates -- tests/circuit_custom_oracle.py against itself, the host-only
calls kzg_circuit_custom_proof_challenges, kzg_circuit_custom_verify_proof and kzg_circuit_custom_blinded_sizes against it
(hashlib, the big-integer oracles, commitments from a known secret: no GPU), and the arithmetic of k_cg_gate replayed on the host
at the magnitudes its bound comment allows (tests/host/cg_reach_host.cpp).

Shapes (n, t, log_ext, exponents): the four smallest of tests/circuit_custom_cases.py and (64, 6, 3, ..), exactly 32 columns at
zeta; plain proofs at all of them, blinded ones where the blinded rule allows."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import blind_oracle as BO
import circuit_custom_cases as CC
import circuit_custom_oracle as CX
import circuit_oracle as CO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import perm_quotient_oracle as PQ
import transcript_oracle as TR
import trapdoor_oracle as TO

R = PQ.R
SECRET = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % R
SHAPES = CC.SHAPES[:4] + [CC.WIDE]
BLINDED = [s for s in SHAPES if s in CC.BLINDED_SHAPES]
INV = K.KZG_ERR_INVALID_ARG
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("beta", "gamma", "alpha", "zeta", "v")
ids = lambda s: "n%d_t%d_e%d_%s" % (s[0], s[1], 1 << s[2], "_".join("".join(map(str, r)) for r in s[3]))


def _proof(oracle, shape, blinded=False, with_pi=True):
    n, t, log_ext, exps = shape

    def make():
        cs = CC.case(n, t, log_ext, exps, with_pi)
        return CX.prove(oracle, cs.cc, log_ext, cs.blinders() if blinded else cs.zero, SECRET)
    return CC.memo(("proof", shape, blinded, with_pi), make)


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


def _challenges(oracle, d, proof=None, key_s=None, exps=None, public=None):
    cc = d["cc"]
    got = K.circuit_custom_proof_challenges(_key(oracle, d, key_s), cc.n, d["log_ext"], cc.exps if exps is None else exps,
                                            _scalars(cc.circuit.ks), _scalars(d["public"] if public is None else public),
                                            d["proof"] if proof is None else proof)
    return tuple(x.v for x in got)


def _verify(oracle, srs, d, proof=None, key_s=None, exps=None, public=None):
    cc = d["cc"]
    return K.circuit_custom_verify_proof(_key(oracle, d, key_s), cc.n, d["log_ext"], cc.exps if exps is None else exps,
                                         _scalars(cc.circuit.ks), _scalars(d["public"] if public is None else public),
                                         d["proof"] if proof is None else proof, srs[0], srs[1])


def _flip(proof, at, bit=1):
    b = bytearray(proof)
    b[at] ^= bit
    return bytes(b)


# ---- the oracle against itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + [(4, 3, 2, ((1, 1, 1),)), (16, 2, 2, ((3, 0), (0, 1))), (8, 5, 3, ((1, 0, 2, 0, 1), (0, 6, 0, 0, 0)))], ids=ids)
def test_oracle_division_degrees_and_the_check_at_a_point(shape):
    n, t, log_ext, exps = shape
    cs = CC.case(n, t, log_ext, exps)
    e, dm = 1 << log_ext, CC.d_max(exps)
    T = cs.quotient  # (asserts a zero remainder and the plain degrees)
    assert len(cs.gprime) <= (dm + 1) * (n - 1) + 1
    assert len(PQ._trim(T)) <= (e - 1) * n
    zetas = (0x1234567, NO.domain_root(NO.log2_exact(n)) if n > 1 else 1)
    for zeta in zetas:
        assert CX.check_at(zeta, T, cs.cc, cs.coefs, CC.ALPHA, CC.BETA, CC.GAMMA)
    zeta = 0xFEDCBA987654321
    r = CX.linearisation(cs.cc, cs.coefs, T, log_ext, cs.zero, CC.ALPHA, CC.BETA, CC.GAMMA, zeta)
    assert not any(r[n:]) and PQ.horner(r, zeta) == 0
    if CC.blinded_legal(*shape):
        bl, coefs, Tb = cs.blinded()  # (asserts deg T~ = max(t n + t + 2, d_max (n + 1) - 1) exactly)
        assert len(PQ._trim(Tb)) == CX.blinded_keep(n, t, dm) if n >= 4 else len(PQ._trim(Tb)) <= CX.blinded_keep(n, t, dm)
        assert len(Tb) == BO.quotient_len(n, t, log_ext) == K.circuit_custom_blinded_sizes(n, t, log_ext, dm)[1]
        for zeta in zetas:
            assert CX.check_at(zeta, Tb, cs.cc, coefs, CC.ALPHA, CC.BETA, CC.GAMMA)
        rb = CX.linearisation(cs.cc, coefs, Tb, log_ext, bl, CC.ALPHA, CC.BETA, CC.GAMMA, zeta)
        assert PQ.horner(rb, zeta) == 0 and rb != r
    else:
        with pytest.raises(K.KzgError):
            K.circuit_custom_blinded_sizes(n, t, log_ext, dm)


@pytest.mark.parametrize("shape", [CC.SBOX, CC.WIDE], ids=ids)
def test_oracle_refuses_a_change_of_one_value(shape):
    n, t, log_ext, exps = shape
    cs = CC.case(n, t, log_ext, exps)
    cc = cs.cc
    zeta = 0xFEDCBA987654321
    row = next(i for i in range(n) if cc.q_custom[0][i])
    wires = [list(col) for col in cc.circuit.wires]
    j = next(j for j in range(t) if cc.exps[0][j])
    wires[j][row] = (wires[j][row] + 1) % R
    qx = [list(col) for col in cc.q_custom]
    qx[0][row] = (qx[0][row] + 1) % R
    ex = [list(r) for r in cc.exps]
    ex[0][j] -= 1 if ex[0][j] > 1 or sum(ex[0]) > 1 else -1
    assert CX.remainder(cc, cs.z, CC.ALPHA, CC.BETA, CC.GAMMA) == []
    for kw in (dict(wires=wires), dict(q_custom=qx), dict(exps=ex)):
        assert CX.remainder(cc, cs.z, CC.ALPHA, CC.BETA, CC.GAMMA, **kw) != [], sorted(kw)
    # and with the true quotient, r_X formed from a changed wire value, selector value or exponent does not vanish at zeta
    T = cs.quotient
    key, wc, zc, pi = cs.coefs
    wc2 = [NO.intt(col) + [0, 0] for col in wires]
    key2 = key[:2 * t + 2] + [NO.intt(col) for col in qx]
    for coefs, ex2 in (((key, wc2, zc, pi), None), ((key2, wc, zc, pi), None), (cs.coefs, ex)):
        r = CX.linearisation(cc, coefs, T, log_ext, cs.zero, CC.ALPHA, CC.BETA, CC.GAMMA, zeta, exps=ex2)
        assert PQ.horner(r, zeta) != 0
    assert PQ.horner(CX.linearisation(cc, cs.coefs, T, log_ext, cs.zero, CC.ALPHA, CC.BETA, CC.GAMMA, zeta), zeta) == 0


# ---- the shape rules -------------------------------------------------------------------------------------------------------------
def test_blinded_sizes_against_the_rule():
    lib = K.load_library()
    seen = set()
    for log_ext in range(0, 5):
        for t in range(1, 9):
            for n in (1, 2, 4, 8, 64):
                for dm in range(0, 9):
                    e = 1 << log_ext
                    legal = 2 <= t <= K.KZG_PQ_MAX_COLUMNS and log_ext <= K.KZG_PQ_MAX_LOG_EXT and e >= max(t + 1, dm + 1) and dm >= 1 and \
                        CX.blinded_ok(n, t, log_ext, dm)
                    nb, lt = C.c_size_t(123), C.c_size_t(456)
                    rc = lib.kzg_circuit_custom_blinded_sizes(n, t, log_ext, dm, C.byref(nb), C.byref(lt))
                    if legal:
                        assert rc == 0 and (nb.value, lt.value) == (2 * t + 3 + e - 2, (e - 1) * n + t + 3), (n, t, log_ext, dm)
                        if dm <= t:  # section 4.24's rule unchanged
                            assert K.circuit_blinded_sizes(n, t, log_ext) == (nb.value, lt.value)
                        seen.add(dm > t)
                    else:
                        assert rc == INV and (nb.value, lt.value) == (123, 456), (n, t, log_ext, dm)
    assert seen == {True, False}
    assert lib.kzg_circuit_custom_blinded_sizes(6, 3, 3, 2, None, None) == INV and lib.kzg_circuit_custom_blinded_sizes(8, 3, 3, 2, None, None) == 0
    assert K.circuit_custom_blinded_sizes(8, 3, 3, 5) == (15, 62)
    with pytest.raises(K.KzgError):
        K.circuit_custom_blinded_sizes(8, 3, 3, 7)  # 7 n + 7 = 63 > L_T = 62
    assert K.circuit_custom_blinded_sizes(8, 3, 3, 6) == (15, 62)  # 54 <= 62, N = 64 >= 55


def test_exports():
    lib = K.load_library()
    for name in ("kzg_circuit_create_custom", "kzg_circuit_custom_gate", "kzg_circuit_custom_quotient", "kzg_circuit_custom_prove",
                 "kzg_circuit_custom_prove_device", "kzg_circuit_custom_proof_challenges", "kzg_circuit_custom_verify_proof",
                 "kzg_circuit_custom_blinded_sizes"):
        assert name in K.ABI_SYMBOLS and hasattr(lib, name), name
    assert K.KZG_ABI_VERSION == 4 == lib.kzg_abi_version()
    assert (K.KZG_CIRCUIT_COL_CUSTOM, K.KZG_CIRCUIT_MAX_CUSTOM) == (96, 8) == (96, CX.MAX_CUSTOM)
    assert K.KZG_CIRCUIT_COL_QLOOKUP < K.KZG_CIRCUIT_COL_CUSTOM
    header = open(os.path.join(HERE, "..", "include", "kzg_mi355x.h")).read()
    assert "#define KZG_CIRCUIT_COL_CUSTOM 96" in header and "#define KZG_CIRCUIT_MAX_CUSTOM 8" in header
    assert "kzg_mi355x/plonk-custom/v1" in header


# ---- the transcript --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_challenges_against_the_oracle(oracle, shape):
    d = _proof(oracle, shape)
    want = tuple(d[k] for k in NAMES)
    assert _challenges(oracle, d) == want and len(set(want)) == 5
    if shape == CC.SBOX:
        d0 = _proof(oracle, shape, with_pi=False)
        assert d0["public"] == [] and _challenges(oracle, d0) == tuple(d0[k] for k in NAMES)
        db = _proof(oracle, shape, blinded=True)
        assert _challenges(oracle, db) == tuple(db[k] for k in NAMES) and db["proof"] != d["proof"]


@pytest.mark.parametrize("shape", [(8, 3, 2, ((1, 1, 1), (3, 0, 0))), (16, 2, 2, ((3, 0), (0, 1)))], ids=ids)
def test_challenges_with_no_one_and_n_public_inputs(oracle, shape):
    """the two ends of the statement's public inputs and one value, at e = t + 1 and at e > t + 1.  The proof's bytes are hashed as
    they are: the same proof serves every statement"""
    n, t, log_ext, exps = shape
    d = _proof(oracle, shape)
    cc = d["cc"]
    assert len(d["public"]) == n
    seen = set()
    for n_public in (0, 1, n):
        public = d["public"][:n_public]
        got = _challenges(oracle, d, public=public)
        assert got == CX.challenges(n, t, log_ext, cc.exps, cc.circuit.ks, d["key48"], public, d["proof"]), n_public
        seen.add(got)
    assert len(seen) == 3 and tuple(d[k] for k in NAMES) in seen


def test_g_an_exponent_and_a_custom_commitment_move_every_challenge(oracle):
    n, t, log_ext, exps = CC.SBOX
    d = _proof(oracle, CC.SBOX)
    cc, base = d["cc"], _challenges(oracle, d)
    moved = lambda got: all(a != b for a, b in zip(got, base))
    # g: one term fewer, the key one commitment shorter
    assert moved(_challenges(oracle, d, key_s=d["key_s"][:-1], exps=cc.exps[:-1]))
    ex = [list(r) for r in cc.exps]
    ex[1][2] += 1
    assert moved(_challenges(oracle, d, exps=ex))
    for j in (2 * t + 2, 2 * t + 3):
        ks = list(d["key_s"])
        ks[j] = (ks[j] + 1) % R
        assert moved(_challenges(oracle, d, key_s=ks))
    pub = list(d["public"])
    pub[-1] = (pub[-1] + 1) % R
    assert moved(_challenges(oracle, d, public=pub))
    # from h1 on the chain is the plain proof's: the fields move what comes after them
    lay = TR.layout(t, log_ext)
    for name, first in {"wires": 0, "z": 2, "chunks": 3, "evals": 4}.items():
        a, b = lay[name]
        got = _challenges(oracle, d, proof=_flip(d["proof"], b - 1))
        assert got[:first] == base[:first] and all(x != y for x, y in zip(got[first:], base[first:])), name
    # the plain statement of the same key prefix gives other challenges
    plain = K.circuit_proof_challenges(_key(oracle, d)[:2 * t + 2], n, log_ext, _scalars(cc.circuit.ks), _scalars(d["public"]), d["proof"])
    assert moved(tuple(x.v for x in plain))


# ---- the verifier ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_verifier_accepts_the_oracles_plain_and_blinded_proofs(oracle, srs, shape):
    n, t, log_ext, exps = shape
    d = _proof(oracle, shape)
    assert len(d["proof"]) == K.circuit_proof_size(t, log_ext)
    assert _verify(oracle, srs, d)
    if shape in BLINDED:
        db = _proof(oracle, shape, blinded=True)
        assert len(db["proof"]) == len(d["proof"]) and db["proof"] != d["proof"] and _verify(oracle, srs, db)
    if shape == CC.SBOX:
        assert _verify(oracle, srs, _proof(oracle, shape, with_pi=False))


def test_verifier_rejects_a_change_in_each_field_the_key_and_the_statement(oracle, srs):
    n, t, log_ext, exps = CC.SBOX
    for blinded in (False, True):
        d = _proof(oracle, CC.SBOX, blinded=blinded)
        cc = d["cc"]
        assert _verify(oracle, srs, d)
        for name, (a, b) in TR.layout(t, log_ext).items():
            if name == "evals":
                for i in range(2 * t):
                    assert not _verify(oracle, srs, d, proof=_flip(d["proof"], a + 32 * i + 31)), (name, i)
            else:
                other = TO.g1_scalar(oracle, 0xABCDEF)
                assert not _verify(oracle, srs, d, proof=d["proof"][:a] + other + d["proof"][a + 48:]), name
        ks = list(d["key_s"])
        ks[2 * t + 2], ks[2 * t + 3] = ks[2 * t + 3], ks[2 * t + 2]  # two custom commitments swapped
        assert ks != d["key_s"] and not _verify(oracle, srs, d, key_s=ks)
        ex = [list(r) for r in cc.exps]
        ex[0][0] -= 1
        assert not _verify(oracle, srs, d, exps=ex)
        ex = [list(r) for r in cc.exps]
        ex[1][1], ex[1][2] = ex[1][2], ex[1][1]
        assert not _verify(oracle, srs, d, exps=ex)
        pub = list(d["public"])
        pub[0] = (pub[0] + 1) % R
        assert not _verify(oracle, srs, d, public=pub)


def test_a_custom_proof_is_no_plain_proof_and_the_other_way_round(oracle, srs):
    n, t, log_ext, exps = CC.SBOX
    d = _proof(oracle, CC.SBOX)
    cc = d["cc"]
    shifts, public = _scalars(cc.circuit.ks), _scalars(d["public"])
    base_key = _key(oracle, d)[:2 * t + 2]
    # the same bytes under the plain verifier of the same key prefix
    assert not K.circuit_verify_proof(base_key, n, log_ext, shifts, public, d["proof"], *srs)
    # the base statement does not hold for these wires, so there is no plain proof of it; a plain proof of a circuit with the same
    # wires, permutation and selectors whose q_C satisfies the base gate is not a custom proof of this key
    c = cc.circuit
    base = CO.Circuit(c.ks, c.wires, c.sigmas, c.q_lin, c.q_mul, [0] * n, c.pi)
    base.q_const = [(-v) % R for v in CO.gate_rows(base)]
    plain = TR.prove(oracle, base, log_ext, BO.Blinders.zero(t, log_ext), SECRET)
    plain_key = [K.G1Point(oracle.p1_mult(oracle.p1_generator(), s)) for s in plain["key_s"]]
    assert K.circuit_verify_proof(plain_key, n, log_ext, shifts, public, plain["proof"], *srs)
    assert len(plain["proof"]) == len(d["proof"])
    assert not _verify(oracle, srs, d, proof=plain["proof"])
    # ... nor of the key made of the plain circuit's commitments and the custom ones
    assert not _verify(oracle, srs, d, proof=plain["proof"], key_s=plain["key_s"] + d["key_s"][2 * t + 2:])


def test_undecodable_bytes_are_invalid_not_an_error(oracle, srs):
    n, t, log_ext, exps = CC.SBOX
    d = _proof(oracle, CC.SBOX)
    lay = TR.layout(t, log_ext)
    for name in ("wires", "z", "chunks", "w"):
        a, _ = lay[name]
        assert not _verify(oracle, srs, d, proof=_flip(d["proof"], a, 0x80)), name  # the compression flag cleared
        assert not _verify(oracle, srs, d, proof=d["proof"][:a] + b"\xff" * 48 + d["proof"][a + 48:]), name
    a, _ = lay["evals"]
    for i in (0, 2 * t - 1):
        assert not _verify(oracle, srs, d, proof=d["proof"][:a + 32 * i] + R.to_bytes(32, "big") + d["proof"][a + 32 * (i + 1):]), i


def test_argument_errors_and_every_shape_rule(oracle, srs):
    n, t, log_ext, exps = CC.SBOX
    g = len(exps)
    d = _proof(oracle, CC.SBOX)
    cc = d["cc"]
    lib = K.load_library()
    rows = np.ascontiguousarray(np.stack([k.p1 for k in _key(oracle, d)]), dtype=np.uint64)
    ks = np.ascontiguousarray(np.stack([K.Scalar(k).limbs() for k in cc.circuit.ks]), dtype=np.uint64)
    pub = np.ascontiguousarray(np.stack([K.Scalar(p).limbs() for p in d["public"]]), dtype=np.uint64)
    buf = np.frombuffer(d["proof"], dtype=np.uint8)
    ex = np.array(cc.exps, dtype=np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    ok = C.c_int(7)

    def verify(rows=rows, n=n, t=t, log_ext=log_ext, g=g, ex=ex, ks=ks, pub=pub, n_public=len(d["public"]), buf=buf, length=len(d["proof"]),
               g1=srs[0], g2=srs[1], valid=C.byref(ok)):
        return lib.kzg_circuit_custom_verify_proof(ptr(rows), n, t, log_ext, g, ptr(ex), ptr(ks), ptr(pub), n_public, ptr(buf), length,
                                                   ptr(g1), 144, ptr(g2), 288, valid)
    assert verify() == 0 and ok.value == 1
    ok.value = 7
    not_fr = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    bad_pub, bad_ks, bad_rows = pub.copy(), ks.copy(), rows.copy()
    bad_pub[1], bad_ks[0] = not_fr, not_fr
    bad_rows[2 * t + 2, 0] ^= 1  # a custom commitment off the curve
    zero_term, big_exp, deg8 = ex.copy(), ex.copy(), ex.copy()
    zero_term[1] = 0       # a term of degree 0 is q_C
    big_exp[1, 0] = 8      # an exponent above 7
    deg8[0] = (5, 2, 1)    # d_max = 8 > e - 1
    for kw in (dict(rows=None), dict(ex=None), dict(ks=None), dict(pub=None), dict(buf=None), dict(g1=None), dict(g2=None), dict(valid=None),
               dict(n=6), dict(t=1), dict(t=8), dict(log_ext=4), dict(g=0), dict(g=9), dict(n_public=n + 1),
               dict(length=len(d["proof"]) - 1), dict(length=len(d["proof"]) + 1), dict(pub=bad_pub), dict(ks=bad_ks), dict(rows=bad_rows),
               dict(ex=zero_term), dict(ex=big_exp), dict(ex=deg8)):
        assert verify(**kw) == INV and ok.value == 7, sorted(kw)
    out = np.zeros((5, 4), dtype=np.uint64)
    args = lambda **kw: [kw.get("rows", ptr(rows)), kw.get("n", n), t, log_ext, kw.get("g", g), kw.get("ex", ptr(ex)), ptr(ks), ptr(pub),
                         len(d["public"]), ptr(buf), kw.get("length", len(d["proof"])), kw.get("out", ptr(out))]
    assert lib.kzg_circuit_custom_proof_challenges(*args()) == 0
    for kw in (dict(rows=None), dict(ex=None), dict(out=None), dict(n=6), dict(g=0), dict(g=9), dict(length=3), dict(ex=ptr(zero_term)),
               dict(ex=ptr(big_exp)), dict(ex=ptr(deg8))):
        assert lib.kzg_circuit_custom_proof_challenges(*args(**kw)) == INV, sorted(kw)
    # e >= d_max + 1 and the column count at zeta: t = 3, e = 4 takes d_max = 3, not 4; t = 6, e = 8 takes g = 3, not 4
    one = np.zeros((5, 4), dtype=np.uint64)
    for tt, le, rows_ex, legal in ((3, 2, [[3, 0, 0]], True), (3, 2, [[2, 1, 1]], False), (6, 3, [[1, 0, 0, 0, 0, 0]] * 3, True),
                                   (6, 3, [[1, 0, 0, 0, 0, 0]] * 4, False), (2, 1, [[1, 0]], False), (2, 2, [[1, 0]] * 8, True)):
        assert CX.shape_ok(tt, le, rows_ex) == legal, (tt, le, rows_ex)
        gg = len(rows_ex)
        key = np.tile(rows[0], (2 * tt + 2 + gg, 1))
        exb = np.array(rows_ex, dtype=np.uint8)
        sh = np.tile(ks[0], (tt, 1))
        proof = np.zeros(TR.proof_size(tt, le) if tt + 1 <= (1 << le) else 64, dtype=np.uint8)
        rc = lib.kzg_circuit_custom_proof_challenges(ptr(key), 8, tt, le, gg, ptr(exb), ptr(sh), None, 0, ptr(proof), len(proof), ptr(one))
        assert (rc == 0) == legal, (tt, le, rows_ex, rc)


# ---- the kernel's arithmetic at the magnitudes its bound comment allows ---------------------------------------------------------
# The bounds the unit's header states (custom_gate_kernels.hip, "Bounds").
RAW_BOUND = (1 << 30) + 4        # |digit 0..7| entering the sum's carry pass (fr30_norm takes 2^31 - 2^29)
NORM_BOUND = (1 << 29) + 4       # |digit 0..7| leaving a carry pass, a load or a product
SUM_TOP_BOUND = 1 << 17          # |digit 8| of the sum of up to 8 terms
PRODUCT_TOP_BOUND = 1 << 14      # |digit 8| of any product (|v| < 0.5002 r)
COLUMN_BOUND = 1 << 62


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_kernel_arithmetic_reaches_its_bounds_on_the_host(tmp_path):
    """tests/host/cg_reach_host.cpp replays k_cg_gate on csrc/fr30.hip.h at canonical extremes and at random values; every
    intermediate stays inside the bound the unit's header states and every result equals the big-integer value"""
    exe = str(tmp_path / "cg_reach_host")
    # -fwrapv: a digit sum that overflowed would wrap on the device, and so must it here
    subprocess.run(["g++", "-O2", "-fwrapv", "-o", exe, os.path.join(HERE, "host", "cg_reach_host.cpp")], check=True)
    import random
    rnd = random.Random(78)
    inv = pow(1 << 256, -1, R)
    extremes = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, (1 << 255) % R, (-(1 << 256)) % R, inv, (-inv) % R]
    img = lambda x: "%064x" % (x * (1 << 256) % R)
    cases = []
    for k in range(96):
        t, g = (7, 8) if k < 32 else (1 + k % 7, 1 + k % 8)
        # images at the extremes: the plain value whose IMAGE is v, so that the digits the kernel loads are the extreme ones
        pick = (lambda: rnd.choice(extremes) * inv % R) if k < 48 else (lambda: rnd.randrange(R))
        exps = [[rnd.randrange(8) for _ in range(t)] for _ in range(g)]
        if k < 16:
            exps = [[7] * t for _ in range(g)]  # the longest chains of products
        for row in exps:
            if sum(row) == 0:
                row[rnd.randrange(t)] = 1
        v = dict(t=t, g=g, exps=exps, f=[pick() for _ in range(t)], qx=[pick() for _ in range(g)])
        if k < 8:  # eight terms of one sign at the largest loaded digits
            v.update(f=[(R - 1) * inv % R] * t, qx=[(R - 1) * inv % R] * g)
        cases.append(v)
    text = "%d\n" % len(cases) + "".join(" ".join([str(v["t"]), str(v["g"])] + [str(p) for row in v["exps"] for p in row] +
                                                  [img(x) for x in v["f"] + v["qx"]]) + "\n" for v in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    rep, res = [int(x) for x in out[:5]], out[5:]
    assert len(res) == len(cases)
    print(dict(zip(["raw sum", "top sum", "norm", "product top", "column"], rep)))
    assert rep[0] <= RAW_BOUND and rep[1] < SUM_TOP_BOUND and rep[2] <= NORM_BOUND and rep[3] < PRODUCT_TOP_BOUND and rep[4] < COLUMN_BOUND, rep
    for k, v in enumerate(cases):
        want = 0
        for s in range(v["g"]):
            m = v["qx"][s]
            for p, x in zip(v["exps"][s], v["f"]):
                m = m * pow(x, p, R) % R
            want = (want + m) % R
        got = int(res[k], 16)
        assert got < R and got * inv % R == want, (k, v)
