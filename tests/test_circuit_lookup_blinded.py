"""CPU: zero-knowledge lookup proofs -- tests/circuit_lookup_blind_oracle.py against itself (exact division,
the degree D, r~_L(zeta) = 0 exactly for the true inputs), the EXISTING kzg_circuit_lookup_verify_proof on the oracle's blinded proofs
under a known secret, and what the new calls do without a device: the shape rule, the blinder draw, NULL pointers, the exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import blind_oracle as BO
import circuit_lookup_blind_oracle as LB
import circuit_lookup_cases as CC
import circuit_lookup_oracle as CL
import kzg_poly_commit_exploration_amd as K
import linearise_oracle as LN
import ntt_oracle as NO
import perm_quotient_oracle as PQ
import trapdoor_oracle as TO

R = PQ.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECRET = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % R
ZETA = 0xFEDCBA987654321
SHAPES = [(4, 2, 1, 2), (8, 3, 3, 2), (1, 2, 1, 3), (2, 3, 2, 3), (64, 6, 1, 3)]
LEGAL = SHAPES[:4] + [(256, 3, 2, 2), (4096, 2, 1, 2), (64, 6, 1, 3)]
REFUSED = [(1, 2, 1, 2), (2, 2, 1, 2), (2, 3, 2, 2)]
NEW_SYMBOLS = ("kzg_circuit_lookup_blinded_sizes", "kzg_circuit_lookup_blinders", "kzg_circuit_lookup_quotient_blinded",
               "kzg_circuit_lookup_prove_blinded", "kzg_circuit_lookup_prove_blinded_device")
ARGS = (CC.THETA, CC.BETA, CC.GAMMA, CC.ALPHA)


def _case(n, t, c, log_ext):
    """(the case, blinders, the blinded coefficients, T~, its chunks) under the module's challenges, built once"""
    def make():
        cs = LB.case(n, t, c, log_ext)
        bl = LB.Blinders.random(t, log_ext, n + t)
        cf = LB.coefficients(cs.lc, cs.z, cs.m, cs.phi, bl)
        T = LB.quotient(cs.lc, cf, log_ext, *ARGS, full_degree=n > 2)  # (asserts a zero remainder)
        return cs, bl, cf, T, LB.chunks(T, n, t, log_ext, bl)
    return CC.memo(("blinded lookup quotient", n, t, c, log_ext), make)


def _proof(oracle, n, t, c, log_ext):
    return CC.memo(("blinded lookup proof", n, t, c, log_ext),
                   lambda: LB.prove(oracle, LB.case(n, t, c, log_ext).lc, log_ext, LB.Blinders.random(t, log_ext, n + t), SECRET))


@pytest.fixture(scope="module")
def srs(oracle):
    """[s^j]G1 for j < 2 and [s^j]G2 for j <= 2"""
    g1 = np.stack([oracle.p1_mult(oracle.p1_generator(), pow(SECRET, j, R)) for j in range(2)])
    g2 = np.stack([K.srs_g2_at(TO.secret_be(SECRET), j) for j in range(3)])
    return g1, g2


def _verify(oracle, srs, d, proof=None):
    lc = d["lc"]
    key = [K.G1Point(oracle.p1_mult(oracle.p1_generator(), s % R)) for s in d["key_s"]]
    return K.circuit_lookup_verify_proof(key, lc.n, d["log_ext"], lc.c, [K.Scalar(x) for x in lc.circuit.ks],
                                         [K.Scalar(x) for x in d["public"]], d["proof"] if proof is None else proof, srs[0], srs[1])


# ---- the oracle against itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t,c,log_ext", SHAPES)
def test_oracle_division_is_exact_and_the_degree_is_as_stated(n, t, c, log_ext):
    cs, bl, cf, T, tc = _case(n, t, c, log_ext)
    e = 1 << log_ext
    D, LT = LB.keep(n, t), BO.quotient_len(n, t, log_ext)
    assert D == max(t * n + t + 3, 3 * n + 2) and D < e * n and D <= LT == (e - 1) * n + t + 3 == len(T)
    assert LB.shape_ok(n, t, c, log_ext) and bl.generic()
    assert not any(T[D:])
    if n > 2:  # (at n <= 2, w^(n + 2) = 1 and the leading terms of phi~(w X) - phi~ and of the permutation cancel)
        assert T[D - 1] != 0
    # the blinded columns' degrees, and which term sets D
    assert len(cf.phi) == n + 3 and cf.phi[-1] and len(cf.m) == n + 2 and cf.m[-1]
    gp, perm = LB.gprime_coeffs(cs.lc, cf, CC.THETA, CC.BETA, CC.ALPHA), BO.numerator(cs.lc.circuit, cf.base, CC.ALPHA, CC.BETA, CC.GAMMA)
    assert len(gp) <= 4 * n + 2 and len(perm) <= (t + 1) * n + t + 3
    if (n, t) == (4, 2):
        assert len(gp) == 4 * n + 2 == D + n and len(perm) - n == t * n + t + 3 < D  # the lookup's term dominates
    if (n, t) == (8, 3):
        assert len(perm) - n == t * n + t + 3 == D and len(gp) - n <= 3 * n + 2 < D  # the permutation's
    # the chunks put T~ back together: sum_c X^(c n) T~_c = T~
    back = [0] * (LT + 1)
    for k, ch in enumerate(tc):
        assert len(ch) == (n + 1 if k < e - 2 else n + t + 3)
        for i, v in enumerate(ch):
            back[k * n + i] = (back[k * n + i] + v) % R
    assert back[:LT] == T and back[LT] == 0
    # all blinders zero: section 4.26's quotient
    zero = LB.Blinders.zero(t, log_ext)
    T0 = LB.quotient(cs.lc, LB.coefficients(cs.lc, cs.z, cs.m, cs.phi, zero), log_ext, *ARGS)
    assert PQ._trim(T0) == PQ._trim(CL.quotient(cs.lc, cs.z, CC.THETA, CC.BETA, CC.GAMMA, CC.ALPHA, cs.m, cs.phi))


@pytest.mark.parametrize("n,t,c,log_ext", SHAPES)
def test_oracle_linearisation_vanishes_at_zeta_exactly_for_the_true_inputs(n, t, c, log_ext):
    cs, bl, cf, T, tc = _case(n, t, c, log_ext)
    lc = cs.lc
    at = lambda cf_, tc_=tc: PQ.horner(LB.linearisation(lc, cf_, tc_, log_ext, *ARGS, ZETA), ZETA)
    r_l = LB.linearisation(lc, cf, tc, log_ext, *ARGS, ZETA)
    assert len(r_l) == n + t + 3 and PQ.horner(r_l, ZETA) == 0
    # one value of a wire, of m, of phi (T~ stays the true quotient)
    row = max(i for i in range(n) if lc.q_lookup[i])
    wires = [list(col) for col in lc.circuit.wires]
    wires[0][row] = (wires[0][row] + 1) % R
    moved = LB.coefficients(lc, cs.z, cs.m, cs.phi, bl)
    moved.base = (moved.base[0], [BO.blind(NO.intt(col), b, n) for col, b in zip(wires, bl.b)], moved.base[2], moved.base[3])
    assert at(moved) != 0
    m2, phi2 = list(cs.m), list(cs.phi)
    m2[0] = (m2[0] + 1) % R
    phi2[n // 2] = (phi2[n // 2] + 1) % R
    assert at(LB.coefficients(lc, cs.z, m2, cs.phi, bl)) != 0
    assert at(LB.coefficients(lc, cs.z, cs.m, phi2, bl)) != 0
    # one blinder of each group that enters r~_L through a polynomial: b, c, p, u
    for group, index in (("b", (0, 1)), ("c", 1), ("p", 2), ("u", 0)):
        other = bl.copy()
        if group == "b":
            other.b[index[0]][index[1]] = (other.b[index[0]][index[1]] + 1) % R
        else:
            getattr(other, group)[index] = (getattr(other, group)[index] + 1) % R
        assert at(LB.coefficients(lc, cs.z, cs.m, cs.phi, other)) != 0, group
    # d: a chunk blinder changed in BOTH chunks it touches cancels (sum_c zeta^(c n) (d_c zeta^n - d_(c-1)) telescopes) ...
    other = bl.copy()
    other.d[0] = (other.d[0] + 1) % R
    assert at(cf, LB.chunks(T, n, t, log_ext, other)) == 0
    # ... and one that a chunk carries at X^n while the next chunk does not take it off does not
    lone = [list(ch) for ch in tc]
    lone[0][n] = (lone[0][n] + 1) % R
    assert at(cf, lone) != 0


@pytest.mark.parametrize("n,t,c,log_ext", SHAPES)
def test_on_the_domain_the_blinded_evaluations_are_the_plain_ones(n, t, c, log_ext):
    cs, bl, cf, T, tc = _case(n, t, c, log_ext)
    w = NO.domain_root(NO.log2_exact(n))
    plain = LN.coefficients(cs.lc.circuit, cs.z)
    for k in {0, n - 1, n // 2}:
        zeta = pow(w, k, R)
        assert LB.evaluations(cs.lc, cf, zeta) == LN.evaluations(cs.lc.circuit, plain, zeta)
        assert LB.lookup_evaluations(cs.lc, cf, zeta) == CL.lookup_evaluations(cs.lc, cs.phi, zeta)
        assert PQ.horner(cf.m, zeta) == cs.m[k] and PQ.horner(cf.phi, zeta) == cs.phi[k]
    assert LB.evaluations(cs.lc, cf, ZETA) != LN.evaluations(cs.lc.circuit, plain, ZETA)


# ---- the existing verifier ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t,c,log_ext", SHAPES)
def test_the_unchanged_verifier_accepts_blinded_proofs_and_rejects_altered_ones(oracle, srs, n, t, c, log_ext):
    d = _proof(oracle, n, t, c, log_ext)
    proof = d["proof"]
    assert len(proof) == K.circuit_lookup_proof_size(t, log_ext, c)
    assert _verify(oracle, srs, d)
    # the blinders are in it: no commitment and no wire or phi evaluation is the plain proof's
    plain = CC.memo(("plain lookup proof", n, t, c, log_ext), lambda: CL.prove(oracle, d["lc"], log_ext, SECRET))
    got, old = CL.split(proof, t, log_ext, c), CL.split(plain["proof"], t, log_ext, c)
    for name in ("wires", "m", "z", "phi", "chunks", "w"):
        assert all(got[name][i:i + 48] != old[name][i:i + 48] for i in range(0, len(got[name]), 48)), name
    assert _verify(oracle, srs, plain)
    # one scalar of every field replaced by another valid one
    lay = CL.layout(t, log_ext, c)
    other = TO.g1_scalar(oracle, 0xABCDEF)
    for name in ("wires", "m", "z", "phi", "chunks", "w"):
        a = lay[name][0]
        assert not _verify(oracle, srs, d, proof[:a] + other + proof[a + 48:]), name
    for k in range(2 * t + c + 2):
        a = lay["evals"][0] + 32 * k
        y = (int.from_bytes(proof[a:a + 32], "big") + 1) % R
        assert not _verify(oracle, srs, d, proof[:a] + y.to_bytes(32, "big") + proof[a + 32:]), k
    # chunks committed under a chunk blinder that r~_L was not formed with
    if n <= 8:
        bl = d["bl"]
        off = bl.copy()
        off.d[0] = (off.d[0] + 1) % R
        forged = CC.memo(("forged lookup proof", n, t, c, log_ext), lambda: LB.prove(oracle, d["lc"], log_ext, bl, SECRET, chunk_bl=off))
        assert not _verify(oracle, srs, forged)


def test_all_blinders_zero_give_the_plain_proof(oracle):
    n, t, c, log_ext = 8, 3, 3, 2
    lc = LB.case(n, t, c, log_ext).lc
    plain = CC.memo(("plain lookup proof", n, t, c, log_ext), lambda: CL.prove(oracle, lc, log_ext, SECRET))
    assert LB.prove(oracle, lc, log_ext, LB.Blinders.zero(t, log_ext), SECRET)["proof"] == plain["proof"]


# ---- the library: what needs no device -------------------------------------------------------------------------------------------
def test_the_shape_rule():
    for n, t, c, log_ext in LEGAL:
        e = 1 << log_ext
        assert K.circuit_lookup_blinded_sizes(n, t, log_ext, c) == (2 * t + e + 6, (e - 1) * n + t + 3), (n, t, c, log_ext)
        assert len(LB.Blinders.zero(t, log_ext).flat()) == 2 * t + e + 6
    for n, t, c, log_ext in REFUSED + [(8, 3, 4, 2), (8, 3, 0, 2), (8, 3, 3, 1), (8, 1, 1, 2), (8, 3, 3, 4), (12, 3, 3, 2), (8, 6, 2, 3)]:
        with pytest.raises(K.KzgError) as ei:
            K.circuit_lookup_blinded_sizes(n, t, log_ext, c)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG, (n, t, c, log_ext)
    lib = K.load_library()
    assert lib.kzg_circuit_lookup_blinded_sizes(8, 3, 2, 3, None, None) == K.KZG_OK
    # every small shape against the rule as the issue writes it
    for n in (1, 2, 4, 8, 16, 64):
        for t in range(1, 9):
            for log_ext in range(0, 5):
                for c in (0, 1, t, t + 1):
                    e = 1 << log_ext
                    D = max(t * n + t + 3, 3 * n + 2)
                    legal = (2 <= t <= K.KZG_PQ_MAX_COLUMNS and log_ext <= K.KZG_PQ_MAX_LOG_EXT and 1 <= c <= t and e >= max(t + 1, 4) and
                             3 * t + e + c + 5 <= 32 and D < e * n and D <= (e - 1) * n + t + 3)
                    nb, lt = C.c_size_t(7), C.c_size_t(7)
                    rc = lib.kzg_circuit_lookup_blinded_sizes(n, t, log_ext, c, C.byref(nb), C.byref(lt))
                    assert (rc == K.KZG_OK) == legal == (legal and LB.shape_ok(n, t, c, log_ext)), (n, t, c, log_ext)
                    assert (nb.value, lt.value) == ((2 * t + e + 6, (e - 1) * n + t + 3) if legal else (7, 7))
                    if legal:  # t <= 6 and e <= 8: at most 16 records of the blinders' tail kernel at zeta
                        assert t + e + 2 <= 16


def test_blinders_are_below_r_and_fresh():
    for t, log_ext in ((2, 2), (3, 2), (2, 3), (6, 3)):
        a, b = K.circuit_lookup_blinders(t, log_ext), K.circuit_lookup_blinders(t, log_ext)
        assert a.shape == (2 * t + (1 << log_ext) + 6, 4) and a.dtype == np.uint64
        for row in list(a) + list(b):
            assert sum(int(x) << (64 * i) for i, x in enumerate(row)) < R
        assert not np.array_equal(a, b)
        assert len({bytes(row) for row in np.concatenate([a, b])}) == 2 * a.shape[0]
    lib = K.load_library()
    out = np.zeros((40, 4), dtype=np.uint64)
    bad = K.KZG_ERR_INVALID_ARG
    assert lib.kzg_circuit_lookup_blinders(3, 2, None) == bad
    for t, log_ext in ((1, 2), (8, 3), (3, 1), (2, 4), (4, 2), (2, 1)):
        assert lib.kzg_circuit_lookup_blinders(t, log_ext, out.ctypes.data) == bad, (t, log_ext)
    assert not out.any()


def test_null_context_and_null_pointers_are_refused():
    lib = K.load_library()
    a = np.zeros((64, 4), dtype=np.uint64)
    p = a.ctypes.data
    bad = K.KZG_ERR_INVALID_ARG
    # ctx, circuit, wires, stride, z, m, phi, PI, four challenges, blinders, out_coeffs, out_p1s
    quot = [p, p, p, 8, p, p, p, None, p, p, p, p, p, p, p]
    # ctx, circuit, key, wires, stride, PI, n_public, blinders, out_proof, bad_row
    prove = [p, p, p, p, 8, None, 0, p, p, None]
    calls = ((lib.kzg_circuit_lookup_quotient_blinded, quot, (3, 7, 13, 14)), (lib.kzg_circuit_lookup_prove_blinded, prove, (4, 5, 6, 9)),
             (lib.kzg_circuit_lookup_prove_blinded_device, prove, (4, 5, 6, 9)))
    # a context that is never read: the pointers are checked first (only the first word, "not a multi-device context", is looked at)
    ctx = np.zeros(1 << 16, dtype=np.uint8).ctypes.data
    for fn, args, optional in calls:
        assert fn(*([None] + args[1:])) == bad, fn.__name__
        for pos in range(1, len(args)):
            if pos in optional:  # sizes; pointers that may be NULL
                continue
            assert fn(*([ctx] + args[1:pos] + [None] + args[pos + 1:])) == bad, (fn.__name__, pos)
    # public inputs announced and not given; bad_row is reset before anything is refused
    row = C.c_size_t(5)
    for fn in (lib.kzg_circuit_lookup_prove_blinded, lib.kzg_circuit_lookup_prove_blinded_device):
        assert fn(ctx, p, p, p, 8, None, 1, p, p, C.byref(row)) == bad and row.value == C.c_size_t(-1).value
        row.value = 5


def test_abi_exports_the_new_symbols():
    lib = K.load_library()
    header = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in K.ABI_SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, header), name
    for name in ("lookup_quotient_blinded", "lookup_prove_blinded", "lookup_prove_blinded_device"):
        assert callable(getattr(K.Circuit, name)), name
    for name in ("circuit_lookup_blinded_sizes", "circuit_lookup_blinders"):
        assert callable(getattr(K, name)) and name in K.__all__, name
    assert K.KZG_ABI_VERSION == 4 == lib.kzg_abi_version()
    assert "LOOKUP PROOFS ARE PLAIN" not in header
    assert "kzg_circuit_lookup_prove are plain; the _blinded forms are zero-knowledge" in header
