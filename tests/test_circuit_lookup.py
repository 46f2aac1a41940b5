"""CPU: circuit proofs with a lookup table -- tests/circuit_lookup_oracle.py against itself, the host-only
calls kzg_circuit_lookup_proof_size, kzg_circuit_lookup_proof_challenges and kzg_circuit_lookup_verify_proof against it (hashlib,
the big-integer oracles, commitments from a known secret: no GPU), and the arithmetic of k_lk_fold / k_lk_constraints replayed on
the host at the magnitudes their bound comments allow (tests/host/lk_reach_host.cpp).

Shapes (n, t, c, log_ext): the three smallest of tests/circuit_lookup_cases.py and (64, 6, 1, 3), exactly 32 columns at zeta."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import circuit_lookup_cases as CC
import circuit_lookup_oracle as CL
import circuit_oracle as CO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import perm_quotient_oracle as PQ
import transcript_oracle as TR
import trapdoor_oracle as TO

R = PQ.R
SECRET = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % R
SHAPES = [(1, 2, 1, 2), (2, 3, 2, 2), (8, 3, 3, 2), (64, 6, 1, 3)]
INV = K.KZG_ERR_INVALID_ARG
HERE = os.path.dirname(os.path.abspath(__file__))


def _proof(oracle, n, t, c, log_ext, with_pi=True):
    return CC.memo(("proof", n, t, c, log_ext, with_pi), lambda: CL.prove(oracle, CC.case(n, t, c, log_ext, with_pi).lc, log_ext, SECRET))


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


def _challenges(oracle, d, proof=None, key_s=None, shifts=None, public=None):
    lc = d["lc"]
    got = K.circuit_lookup_proof_challenges(_key(oracle, d, key_s), lc.n, d["log_ext"], lc.c,
                                            _scalars(lc.circuit.ks if shifts is None else shifts),
                                            _scalars(d["public"] if public is None else public), d["proof"] if proof is None else proof)
    return tuple(x.v for x in got)


def _verify(oracle, srs, d, proof=None, key_s=None, public=None):
    lc = d["lc"]
    return K.circuit_lookup_verify_proof(_key(oracle, d, key_s), lc.n, d["log_ext"], lc.c, _scalars(lc.circuit.ks),
                                         _scalars(d["public"] if public is None else public), d["proof"] if proof is None else proof,
                                         srs[0], srs[1])


def _flip(proof, at, bit=1):
    b = bytearray(proof)
    b[at] ^= bit
    return bytes(b)


# ---- the oracle against itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t,c,log_ext", SHAPES + [(4, 3, 2, 2), (8, 2, 2, 2), (16, 3, 1, 2), (8, 5, 3, 3)])
def test_oracle_division_degrees_and_the_check_at_a_point(n, t, c, log_ext):
    cs = CC.case(n, t, c, log_ext)
    e = 1 << log_ext
    T = cs.quotient  # (asserts a zero remainder)
    assert len(cs.gprime) <= 4 * (n - 1) + 1  # deg G' <= 4 (n - 1)
    assert len(T) <= (e - 1) * n
    for zeta in (0x1234567, NO.domain_root(NO.log2_exact(n)) if n > 1 else 1):
        assert CL.check_at(zeta, T, cs.lc, cs.z, CC.THETA, CC.BETA, CC.GAMMA, CC.ALPHA, cs.m, cs.phi)
    zeta = 0xFEDCBA987654321
    r_l = CL.linearisation(cs.lc, cs.z, T, log_ext, CC.THETA, CC.BETA, CC.GAMMA, CC.ALPHA, zeta, cs.m, cs.phi)
    assert len(r_l) == n and PQ.horner(r_l, zeta) == 0


@pytest.mark.parametrize("n,t,c,log_ext", [(8, 3, 3, 2), (64, 6, 1, 3)])
def test_oracle_refuses_a_change_of_one_value(n, t, c, log_ext):
    cs = CC.case(n, t, c, log_ext)
    lc = cs.lc
    args = (CC.THETA, CC.BETA, CC.GAMMA, CC.ALPHA)
    zeta = 0xFEDCBA987654321
    row = max(i for i in range(n) if lc.q_lookup[i])

    def r_l_at_zeta(m=cs.m, phi=cs.phi, wires=None, table=None):
        """r_L(zeta) with T the quotient part of the numerator's division (the remainder dropped)"""
        num = CO.numerator(lc.circuit, cs.z, CC.ALPHA, CC.BETA, CC.GAMMA, wires,
                           extra=CL.gprime_coeffs(lc, CC.THETA, CC.BETA, CC.ALPHA, m, phi, wires, table))
        T, rem = PQ.divide_vanishing(num, n)
        return rem, T

    assert r_l_at_zeta()[0] == []
    m2, phi2 = list(cs.m), list(cs.phi)
    m2[next(i for i in range(n) if cs.m[i])] += 1
    phi2[n // 2] = (phi2[n // 2] + 1) % R
    wires = [list(col) for col in lc.circuit.wires]
    wires[0][row] = (wires[0][row] + 1) % R
    table = [list(col) for col in lc.table]
    table[0][0] = (table[0][0] + 1) % R
    for kw in (dict(m=m2), dict(phi=phi2), dict(wires=wires), dict(table=table)):
        rem, T = r_l_at_zeta(**kw)
        assert rem != [], sorted(kw)
    # and with the true quotient, r_L formed from a changed m or phi does not vanish at zeta
    for kw in (dict(m=m2), dict(phi=phi2)):
        r_l = CL.linearisation(lc, cs.z, cs.quotient, log_ext, *args[:3], CC.ALPHA, zeta, kw.get("m", cs.m), kw.get("phi", cs.phi))
        assert PQ.horner(r_l, zeta) != 0, sorted(kw)


# ---- the format ------------------------------------------------------------------------------------------------------------------
def test_proof_size_against_the_formula_and_the_shape_rules():
    lib = K.load_library()
    for log_ext in range(0, 5):
        for t in range(0, 9):
            for c in range(0, 9):
                e = 1 << log_ext
                legal = 2 <= t <= K.KZG_PQ_MAX_COLUMNS and log_ext <= K.KZG_PQ_MAX_LOG_EXT and e >= max(t + 1, 4) and 1 <= c <= t and \
                    3 * t + e + c + 5 <= 32
                out = C.c_size_t(12345)
                rc = lib.kzg_circuit_lookup_proof_size(t, log_ext, c, C.byref(out))
                if legal:
                    assert rc == 0 and out.value == 48 * (t + e + 3) + 32 * (2 * t + c + 2) == CL.proof_size(t, log_ext, c), (t, log_ext, c)
                else:
                    assert rc == INV and out.value == 12345, (t, log_ext, c)
    assert K.circuit_lookup_proof_size(3, 2, 3) == 832
    assert lib.kzg_circuit_lookup_proof_size(3, 2, 3, None) == INV
    assert K.circuit_lookup_proof_size(6, 3, 1) and lib.kzg_circuit_lookup_proof_size(6, 3, 2, C.byref(C.c_size_t())) == INV  # 32 / 33 columns


def test_exports():
    lib = K.load_library()
    for name in ("kzg_circuit_create_lookup", "kzg_circuit_lookup_columns", "kzg_circuit_lookup_quotient", "kzg_circuit_lookup_prove",
                 "kzg_circuit_lookup_prove_device", "kzg_circuit_lookup_proof_size", "kzg_circuit_lookup_proof_challenges",
                 "kzg_circuit_lookup_verify_proof"):
        assert name in K.ABI_SYMBOLS and hasattr(lib, name), name
    assert K.KZG_ABI_VERSION == 4 == lib.kzg_abi_version()
    assert (K.KZG_CIRCUIT_COL_TABLE, K.KZG_CIRCUIT_COL_QLOOKUP) == (64, 80)
    assert K.KZG_CIRCUIT_COL_L0 < K.KZG_CIRCUIT_COL_TABLE and K.KZG_CIRCUIT_COL_TABLE + K.KZG_PQ_MAX_COLUMNS <= K.KZG_CIRCUIT_COL_QLOOKUP
    header = open(os.path.join(HERE, "..", "include", "kzg_mi355x.h")).read()
    assert "NOT zero-knowledge" in header and "#define KZG_CIRCUIT_COL_TABLE 64" in header and "#define KZG_CIRCUIT_COL_QLOOKUP 80" in header


# ---- the transcript --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t,c,log_ext", SHAPES)
def test_challenges_against_the_oracle(oracle, n, t, c, log_ext):
    d = _proof(oracle, n, t, c, log_ext)
    want = tuple(d[k] for k in ("theta", "beta", "gamma", "alpha", "zeta", "v"))
    assert _challenges(oracle, d) == want and len(set(want)) == 6
    if n == 8:
        d0 = _proof(oracle, n, t, c, log_ext, with_pi=False)
        assert d0["public"] == [] and _challenges(oracle, d0) == tuple(d0[k] for k in ("theta", "beta", "gamma", "alpha", "zeta", "v"))


@pytest.mark.parametrize("n,t,c,log_ext", [(8, 3, 3, 2), (16, 2, 1, 2)])
def test_challenges_with_no_one_and_n_public_inputs(oracle, n, t, c, log_ext):
    """the two ends of the statement's public inputs and one value, at e = t + 1 and at e > t + 1.  The proof's bytes are hashed as
    they are: the same proof serves every statement"""
    d = _proof(oracle, n, t, c, log_ext)
    lc = d["lc"]
    assert len(d["public"]) == n
    seen = set()
    for n_public in (0, 1, n):
        public = d["public"][:n_public]
        got = _challenges(oracle, d, public=public)
        assert got == CL.challenges(n, t, log_ext, c, lc.circuit.ks, d["key48"], public, d["proof"]), n_public
        seen.add(got)
    assert len(seen) == 3 and tuple(d[k] for k in ("theta", "beta", "gamma", "alpha", "zeta", "v")) in seen


def test_every_field_moves_the_challenges_after_it_and_none_before(oracle):
    n, t, c, log_ext = 8, 3, 3, 2
    d = _proof(oracle, n, t, c, log_ext)
    lc, base = d["lc"], _challenges(oracle, d)

    def changed(got, first):
        """the challenges from index `first` on differ (theta, beta, gamma, alpha, zeta, v), the earlier ones do not"""
        assert got[:first] == base[:first], (first, "an earlier challenge moved")
        assert all(a != b for a, b in zip(got[first:], base[first:])), (first, "a later challenge stayed")

    for j in (0, t + 1, 2 * t + 1, 2 * t + 2, 2 * t + c + 2):  # the statement: everything moves; the table and q_K are in it
        ks = list(d["key_s"])
        ks[j] = (ks[j] + 1) % R
        changed(_challenges(oracle, d, key_s=ks), 0)
    sh = list(lc.circuit.ks)
    sh[t - 1] = (sh[t - 1] + 1) % R
    changed(_challenges(oracle, d, shifts=sh), 0)
    pub = list(d["public"])
    pub[-1] = (pub[-1] + 1) % R
    changed(_challenges(oracle, d, public=pub), 0)
    changed(_challenges(oracle, d, public=d["public"][:-1]), 0)  # n_public alone
    lay = CL.layout(t, log_ext, c)
    first = {"wires": 0, "m": 1, "z": 3, "phi": 3, "chunks": 4, "evals": 5}
    for name, k in first.items():
        a, b = lay[name]
        for at in (a, b - 1):
            changed(_challenges(oracle, d, proof=_flip(d["proof"], at)), k)
    a, b = lay["w"]
    assert _challenges(oracle, d, proof=_flip(d["proof"], a)) == base  # W comes after every challenge
    # c is in the statement: the same bytes under another c have another length, and are refused
    with pytest.raises(K.KzgError):
        K.circuit_lookup_proof_challenges(_key(oracle, d)[:-1], n, log_ext, c - 1, _scalars(lc.circuit.ks), _scalars(d["public"]), d["proof"])


# ---- the verifier ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t,c,log_ext", SHAPES)
def test_verifier_accepts_the_oracles_proofs(oracle, srs, n, t, c, log_ext):
    d = _proof(oracle, n, t, c, log_ext)
    assert len(d["proof"]) == K.circuit_lookup_proof_size(t, log_ext, c)
    assert _verify(oracle, srs, d)
    if n == 8:
        assert _verify(oracle, srs, _proof(oracle, n, t, c, log_ext, with_pi=False))


def test_verifier_rejects_a_change_in_each_field_the_key_and_the_statement(oracle, srs):
    n, t, c, log_ext = 8, 3, 3, 2
    d = _proof(oracle, n, t, c, log_ext)
    assert _verify(oracle, srs, d)
    lay = CL.layout(t, log_ext, c)
    for name, (a, b) in lay.items():
        if name == "evals":
            for i in range(2 * t + c + 2):  # every evaluation: its last byte (the value stays canonical or stops decoding)
                assert not _verify(oracle, srs, d, proof=_flip(d["proof"], a + 32 * i + 31)), (name, i)
        else:
            # another valid point in the field: the generator's multiple in place of the first commitment of the field
            other = TO.g1_scalar(oracle, 0xABCDEF)
            assert not _verify(oracle, srs, d, proof=d["proof"][:a] + other + d["proof"][a + 48:]), name
    ks = list(d["key_s"])
    ks[2 * t + 2], ks[2 * t + 3] = ks[2 * t + 3], ks[2 * t + 2]  # two table commitments swapped
    assert ks != d["key_s"] and not _verify(oracle, srs, d, key_s=ks)
    ks = list(d["key_s"])
    ks[2 * t + c + 2] = (ks[2 * t + c + 2] + 1) % R  # q_K
    assert not _verify(oracle, srs, d, key_s=ks)
    pub = list(d["public"])
    pub[0] = (pub[0] + 1) % R
    assert not _verify(oracle, srs, d, public=pub)


def test_a_plain_proof_of_the_same_circuit_is_no_lookup_proof(oracle, srs):
    import blind_oracle as BO
    n, t, c, log_ext = 8, 3, 3, 2
    d = _proof(oracle, n, t, c, log_ext)
    lc = d["lc"]
    plain = TR.prove(oracle, lc.circuit, log_ext, BO.Blinders.zero(t, log_ext), SECRET)
    lib = K.load_library()
    assert len(plain["proof"]) != len(d["proof"])
    rows = np.ascontiguousarray(np.stack([k.p1 for k in _key(oracle, d)]), dtype=np.uint64)
    ks = np.ascontiguousarray(np.stack([K.Scalar(k).limbs() for k in lc.circuit.ks]), dtype=np.uint64)
    pub = np.ascontiguousarray(np.stack([K.Scalar(p).limbs() for p in d["public"]]), dtype=np.uint64)
    ok = C.c_int(7)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def run(buf):
        b = np.frombuffer(buf, dtype=np.uint8)
        return lib.kzg_circuit_lookup_verify_proof(ptr(rows), n, t, log_ext, c, ptr(ks), ptr(pub), len(d["public"]), ptr(b), len(buf),
                                                   ptr(srs[0]), 144, ptr(srs[1]), 288, C.byref(ok))
    assert run(plain["proof"]) == INV and ok.value == 7  # another length
    # padded to the lookup proof's length with valid encodings (points at infinity, zero scalars): it decodes, and is refused
    lay = CL.layout(t, log_ext, c)
    padded = bytearray(d["proof"])
    padded[:len(plain["proof"]) - 48] = plain["proof"][:-48]
    padded[lay["w"][0]:] = plain["proof"][-48:]
    assert run(bytes(padded)) == 0 and ok.value == 0
    assert run(d["proof"]) == 0 and ok.value == 1
    # and the lookup proof is no plain proof
    with pytest.raises(K.KzgError):
        K.circuit_verify_proof(_key(oracle, d)[:2 * t + 2], n, log_ext, _scalars(lc.circuit.ks), _scalars(d["public"]), d["proof"], *srs)


def test_undecodable_bytes_are_invalid_not_an_error(oracle, srs):
    n, t, c, log_ext = 8, 3, 3, 2
    d = _proof(oracle, n, t, c, log_ext)
    lay = CL.layout(t, log_ext, c)
    for name in ("wires", "m", "z", "phi", "chunks", "w"):
        a, _ = lay[name]
        assert not _verify(oracle, srs, d, proof=_flip(d["proof"], a, 0x80)), name  # the compression flag cleared
        assert not _verify(oracle, srs, d, proof=d["proof"][:a] + b"\xff" * 48 + d["proof"][a + 48:]), name
    a, _ = lay["evals"]
    for i in (0, 2 * t + c + 1):
        assert not _verify(oracle, srs, d, proof=d["proof"][:a + 32 * i] + R.to_bytes(32, "big") + d["proof"][a + 32 * (i + 1):]), i


def test_argument_errors(oracle, srs):
    n, t, c, log_ext = 8, 3, 3, 2
    d = _proof(oracle, n, t, c, log_ext)
    lc = d["lc"]
    lib = K.load_library()
    rows = np.ascontiguousarray(np.stack([k.p1 for k in _key(oracle, d)]), dtype=np.uint64)
    ks = np.ascontiguousarray(np.stack([K.Scalar(k).limbs() for k in lc.circuit.ks]), dtype=np.uint64)
    pub = np.ascontiguousarray(np.stack([K.Scalar(p).limbs() for p in d["public"]]), dtype=np.uint64)
    buf = np.frombuffer(d["proof"], dtype=np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    ok = C.c_int(7)

    def verify(rows=rows, n=n, t=t, log_ext=log_ext, c=c, ks=ks, pub=pub, n_public=len(d["public"]), buf=buf, length=len(d["proof"]),
               g1=srs[0], g2=srs[1], valid=C.byref(ok)):
        return lib.kzg_circuit_lookup_verify_proof(ptr(rows), n, t, log_ext, c, ptr(ks), ptr(pub), n_public, ptr(buf), length, ptr(g1), 144,
                                                   ptr(g2), 288, valid)
    assert verify() == 0 and ok.value == 1
    ok.value = 7
    not_fr = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    bad_pub, bad_ks, bad_rows = pub.copy(), ks.copy(), rows.copy()
    bad_pub[1], bad_ks[0] = not_fr, not_fr
    bad_rows[2 * t + 2, 0] ^= 1  # a table commitment off the curve
    for kw in (dict(rows=None), dict(ks=None), dict(pub=None), dict(buf=None), dict(g1=None), dict(g2=None), dict(valid=None),
               dict(n=6), dict(t=1), dict(t=8), dict(log_ext=4), dict(c=0), dict(c=4), dict(n_public=n + 1), dict(length=len(d["proof"]) - 1),
               dict(length=len(d["proof"]) + 1), dict(pub=bad_pub), dict(ks=bad_ks), dict(rows=bad_rows)):
        assert verify(**kw) == INV and ok.value == 7, sorted(kw)
    out = np.zeros((6, 4), dtype=np.uint64)
    args = lambda **kw: [kw.get("rows", ptr(rows)), kw.get("n", n), t, log_ext, kw.get("c", c), ptr(ks), ptr(pub), len(d["public"]), ptr(buf),
                         kw.get("length", len(d["proof"])), kw.get("out", ptr(out))]
    assert lib.kzg_circuit_lookup_proof_challenges(*args()) == 0
    for kw in (dict(rows=None), dict(out=None), dict(n=6), dict(c=0), dict(c=4), dict(length=3)):
        assert lib.kzg_circuit_lookup_proof_challenges(*args(**kw)) == INV, sorted(kw)


# ---- the kernels' arithmetic at the magnitudes their bound comments allow -------------------------------------------------------
# The bounds the unit's header states (lookup_circuit_kernels.hip, "Bounds"), per sum in the order the replay reports them: the folded
# sums s_f / s_t, F, Tt, D, E, W.
RAW_BOUND = (1 << 30) + 8        # |digit 0..7| entering a carry pass (fr30_norm takes 2^31 - 2^29)
NORM_BOUND = (1 << 29) + 4       # |digit 0..7| leaving a carry pass, a load or a product
TOP_BOUNDS = {"fold": 1 << 17, "F": 2 * 0x73EE, "Tt": 1 << 18, "D": 0x73EE + 1, "E": 2 * 0x73EE, "W": 1 << 18}
COLUMN_BOUND = 1 << 62


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_kernel_arithmetic_reaches_its_bounds_on_the_host(tmp_path):
    """tests/host/lk_reach_host.cpp replays k_lk_fold and k_lk_constraints on csrc/fr30.hip.h at canonical extremes and at random
    values; every intermediate stays inside the bound the unit's header states and every result equals the big-integer value"""
    exe = str(tmp_path / "lk_reach_host")
    # -fwrapv: a digit sum that overflowed would wrap on the device, and so must it here
    subprocess.run(["g++", "-O2", "-fwrapv", "-o", exe, os.path.join(HERE, "host", "lk_reach_host.cpp")], check=True)
    import random
    rnd = random.Random(77)
    extremes = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, (1 << 255) % R, (-(1 << 256)) % R, pow(1 << 256, -1, R), (-pow(1 << 256, -1, R)) % R]
    img = lambda x: "%064x" % (x * (1 << 256) % R)
    names = ("theta", "beta", "alpha", "qk", "l0", "m", "phi", "phir")
    cases = []
    for k in range(96):
        c = 7 if k < 32 else 1 + k % 7
        # images at the extremes: the plain value whose IMAGE is v, so that the digits the kernel loads are the extreme ones
        pick = (lambda: rnd.choice(extremes) * pow(1 << 256, -1, R) % R) if k < 48 else (lambda: rnd.randrange(R))
        v = {name: pick() for name in names}
        v.update(c=c, f=[pick() for _ in range(c)], tab=[pick() for _ in range(c)])
        if k < 16:  # the largest folded sums: every column and every power of theta at r - 1
            v.update(theta=R - 1, f=[R - 1] * c, tab=[R - 1] * c)
        cases.append(v)
    text = "%d\n" % len(cases) + "".join(" ".join([str(v["c"])] + [img(v[name]) for name in names] + [img(x) for x in v["f"] + v["tab"]]) + "\n"
                                         for v in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    rep, res = [int(x) for x in out[:15]], out[15:]
    assert len(res) == 3 * len(cases)
    sums = ("fold", "F", "Tt", "D", "E", "W")
    print(dict(zip(["raw " + x for x in sums] + ["top " + x for x in sums] + ["norm", "product top", "column"], rep)))
    for i, name in enumerate(sums):
        assert rep[i] <= RAW_BOUND, (name, rep[i])
        assert rep[6 + i] < TOP_BOUNDS[name], (name, rep[6 + i])
    assert rep[12] <= NORM_BOUND and rep[13] <= 0x73EE // 2 + 2 and rep[14] < COLUMN_BOUND, rep[12:]
    inv = pow(1 << 256, -1, R)
    for k, v in enumerate(cases):
        th = [pow(v["theta"], j, R) for j in range(v["c"])]
        sf = sum(a * b for a, b in zip(th, v["f"])) % R
        st = sum(a * b for a, b in zip(th, v["tab"])) % R
        f, T = v["qk"] * sf % R, st
        F, Tt = (v["beta"] + f) % R, (v["beta"] + T) % R
        lk1 = ((v["phir"] - v["phi"]) * F % R * Tt - Tt + v["m"] * F) % R
        gp = (pow(v["alpha"], 3, R) * lk1 + pow(v["alpha"], 4, R) * v["l0"] % R * v["phi"]) % R
        got = [int(x, 16) for x in res[3 * k:3 * k + 3]]
        assert all(x < R for x in got) and [x * inv % R for x in got] == [f, T, gp], (k, v)
