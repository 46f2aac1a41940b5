"""CPU: zero-knowledge circuit proofs -- tests/blind_oracle.py against itself, the EXISTING
kzg_circuit_verify on blinded proofs made from the known secret (commitments [P(s)]G and the proof [h(s)]G: no GPU, no new library
code -- the proof that the verifier need not change), kzg_circuit_blinders, the errors of the new calls that are answered before any
device is touched, and the export of every new symbol."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import blind_oracle as BO
import circuit_oracle as CO
import kzg_poly_commit_exploration_amd as K
import linearise_oracle as LO
import ntt_oracle as NO
import perm_quotient_oracle as PQ
import trapdoor_oracle as TO

R = PQ.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA, BETA, GAMMA = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % R, 0x1F2E3D4C5B6A79881F2E3D4C5B6A7988 % R, 0x123456789ABCDEF0FEDCBA9876543210 % R
ZETA, V = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R, 0x6A09E667F3BCC908B2FB1366EA957D3E3ADEC17512775099DA2F590B0667322A % R
SECRET = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % R
NEW_SYMBOLS = ("kzg_circuit_blinded_sizes", "kzg_circuit_blinders", "kzg_blind_evaluations", "kzg_commit_evaluations_blinded",
               "kzg_circuit_quotient_blinded", "kzg_circuit_quotient_blinded_device", "kzg_circuit_open_blinded",
               "kzg_circuit_open_blinded_device")
SHAPES = [(3, 3, 2), (4, 2, 2), (4, 7, 3)]  # (8, 3, 2), (16, 2, 2), (16, 7, 3) as (log n, t, log_ext)

_CACHE = {}


def _case(k, t, log_ext):
    """a satisfied circuit with its z, blinders, blinded coefficients and T~, computed once"""
    key = (k, t, log_ext)
    if key not in _CACHE:
        c = CO.satisfied(k, t, 500 + 10 * k + t, True)
        z, last = CO.z_of(c, BETA, GAMMA)
        assert last == 1
        bl = BO.Blinders.random(t, log_ext, 10 * k + t)
        coefs = BO.coefficients(c, z, bl)
        _CACHE[key] = (c, z, bl, coefs, BO.quotient(c, coefs, log_ext, ALPHA, BETA, GAMMA))
    return _CACHE[key]


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,t,log_ext", SHAPES)
def test_oracle_division_is_exact_and_the_degree_is_as_stated(k, t, log_ext):
    c, z, bl, coefs, T = _case(k, t, log_ext)
    n = c.n
    assert BO.shape_ok(n, t, log_ext) and len(T) == BO.quotient_len(n, t, log_ext)
    assert len(PQ._trim(T)) == t * n + t + 3  # deg T~ = t n + t + 2
    # the blinded columns agree with the plain ones on H
    w = NO.domain_root(k)
    for f, col in zip(coefs[1], c.wires):
        assert len(f) == n + 2 and [PQ.horner(f, pow(w, i, R)) for i in range(n)] == list(col)
    assert len(coefs[2]) == n + 3 and [PQ.horner(coefs[2], pow(w, i, R)) for i in range(n)] == list(z)
    # the chunks recombine to T~ whatever the chunk blinders
    tc = BO.chunks(T, n, t, log_ext, bl)
    assert [len(ch) for ch in tc] == [n + 1] * ((1 << log_ext) - 2) + [n + t + 3]
    for x in (ZETA, SECRET):
        assert sum(pow(x, i * n, R) * PQ.horner(ch, x) for i, ch in enumerate(tc)) % R == PQ.horner(T, x)
    # and T~ is the quotient: T~(x) Z_H(x) == Num(x) at a point of no domain
    num = BO.numerator(c, coefs, ALPHA, BETA, GAMMA)
    assert PQ.horner(T, ZETA) * (pow(ZETA, n, R) - 1) % R == PQ.horner(num, ZETA)


@pytest.mark.parametrize("k,t,log_ext", SHAPES)
def test_oracle_linearisation_vanishes_at_zeta_exactly_for_the_true_inputs(k, t, log_ext):
    c, z, bl, coefs, T = _case(k, t, log_ext)
    n = c.n
    w = NO.domain_root(k)
    for zeta in (ZETA, 12345, w, 1):
        r = BO.linearisation(c, coefs, T, log_ext, bl, ALPHA, BETA, GAMMA, zeta)
        assert len(r) == n + t + 3 and PQ.horner(r, zeta) == 0, zeta
    # zeta in H: Z = 0, so the blinded evaluations are the plain ones
    plain = LO.coefficients(c, z)
    for zeta in (1, w, pow(w, n - 1, R)):
        assert BO.evaluations(c, coefs, zeta) == LO.evaluations(c, plain, zeta)
    assert BO.evaluations(c, coefs, ZETA) != LO.evaluations(c, plain, ZETA)
    # one wire value changed (T~, z and the blinders stay)
    wires = [list(col) for col in c.wires]
    wires[t - 1][n - 1] = (wires[t - 1][n - 1] + 1) % R
    other = CO.Circuit(c.ks, wires, c.sigmas, c.q_lin, c.q_mul, c.q_const, c.pi)
    assert PQ.horner(BO.linearisation(other, BO.coefficients(other, z, bl), T, log_ext, bl, ALPHA, BETA, GAMMA, ZETA), ZETA) != 0
    # one coefficient of T~ changed: a low one, and the top one of the last chunk
    for at in (0, t * n + t + 2):
        bad = list(T)
        bad[at] = (bad[at] + 1) % R
        assert PQ.horner(BO.linearisation(c, coefs, bad, log_ext, bl, ALPHA, BETA, GAMMA, ZETA), ZETA) != 0, at
    # one blinder changed, T~ kept: a wire's, z's
    for group, i in (("b", 0), ("c", 2)):
        other_bl = BO.Blinders(bl.b, bl.c, bl.d)
        if group == "b":
            other_bl.b[t - 1][1] = (other_bl.b[t - 1][1] + 1) % R
        else:
            other_bl.c[i] = (other_bl.c[i] + 1) % R
        oc = BO.coefficients(c, z, other_bl)
        assert PQ.horner(BO.linearisation(c, oc, T, log_ext, other_bl, ALPHA, BETA, GAMMA, ZETA), ZETA) != 0, group
    # a chunk blinder changes the chunks and r~, never r~(zeta): sum zeta^(c n) T~_c = T~
    other_bl = BO.Blinders(bl.b, bl.c, [(d + 1) % R for d in bl.d])
    r2 = BO.linearisation(c, coefs, T, log_ext, other_bl, ALPHA, BETA, GAMMA, ZETA)
    assert r2 != BO.linearisation(c, coefs, T, log_ext, bl, ALPHA, BETA, GAMMA, ZETA) and PQ.horner(r2, ZETA) == 0


def test_oracle_patch_where_the_index_ranges_overlap():
    for n in (1, 2):
        f = [11 * (i + 1) for i in range(n)]
        b = [3, 5, 7]
        got = BO.blind(f, b, n)
        for x in (2, ZETA):
            assert PQ.horner(got, x) == (PQ.horner(f, x) + PQ.horner(b, x) * (pow(x, n, R) - 1)) % R


def test_oracle_refuses_an_unsatisfied_gate():
    c, z, bl, coefs, T = _case(3, 3, 2)
    q_const = list(c.q_const)
    q_const[2] = (q_const[2] + 1) % R
    other = CO.Circuit(c.ks, c.wires, c.sigmas, c.q_lin, c.q_mul, q_const, c.pi)
    _, rem = BO.quotient(other, BO.coefficients(other, z, bl), 2, ALPHA, BETA, GAMMA, exact=False)
    assert rem != []


# ---- the existing verifier on blinded proofs made from the secret ----------------------------------------------------------------
def _point(oracle, v):
    return K.G1Point(oracle.p1_mult(oracle.p1_generator(), v % R))


@pytest.fixture(scope="module")
def srs(oracle):
    """[s^j]G1 for j < 2 and [s^j]G2 for j <= 2"""
    g1 = np.stack([oracle.p1_mult(oracle.p1_generator(), pow(SECRET, j, R)) for j in range(2)])
    g2 = np.stack([K.srs_g2_at(TO.secret_be(SECRET), j) for j in range(3)])
    return g1, g2


def _verify(d, srs, oracle, **changes):
    d = dict(d, **changes)
    c = d["c"]
    pts = lambda scalars: [_point(oracle, s) for s in scalars]
    abar, sbar, zw = d["evals"]
    ev = ([K.Scalar(a) for a in abar], [K.Scalar(s) for s in sbar], K.Scalar(zw))
    last = max(i for i, p in enumerate(c.pi) if p)
    return K.circuit_verify(pts(d["key_s"]), c.n, d["log_ext"], [K.Scalar(k) for k in c.ks], pts(d["wire_s"]), _point(oracle, d["z_s"]),
                            pts(d["t_s"]), [K.Scalar(p) for p in c.pi[:last + 1]], ev, K.Scalar(ALPHA), K.Scalar(BETA),
                            K.Scalar(GAMMA), K.Scalar(d["zeta"]), K.Scalar(d["v"]), _point(oracle, d["w"]), srs[0], srs[1])


@pytest.mark.parametrize("k,t,log_ext", SHAPES)
def test_the_unchanged_verifier_accepts_blinded_proofs_and_rejects_altered_ones(oracle, srs, k, t, log_ext):
    c, z, bl, _, _ = _case(k, t, log_ext)
    d = BO.proof_case(c, z, log_ext, bl, ALPHA, BETA, GAMMA, ZETA, V, SECRET)
    assert d["ys"][0] == [0] and PQ.horner(d["r"], ZETA) == 0
    assert _verify(d, srs, oracle)
    # the commitments are not those of the plain polynomials
    plain = LO.coefficients(c, z)
    assert d["wire_s"] != [PQ.horner(col, SECRET) for col in plain[1]] and d["z_s"] != PQ.horner(plain[2], SECRET)
    # one commitment: a wire's, z's, a chunk's
    for name, j in (("wire_s", 0), ("wire_s", t - 1), ("t_s", 0), ("t_s", (1 << log_ext) - 2)):
        s = list(d[name])
        s[j] = (s[j] + 1) % R
        assert not _verify(d, srs, oracle, **{name: s}), (name, j)
    assert not _verify(d, srs, oracle, z_s=(d["z_s"] + 1) % R)
    # one evaluation
    abar, sbar, zw = d["evals"]
    for j in sorted({0, t - 1}):
        bad = list(abar)
        bad[j] = (bad[j] + 1) % R
        assert not _verify(d, srs, oracle, evals=(bad, sbar, zw)), j
    assert not _verify(d, srs, oracle, evals=(abar, [(sbar[0] + 1) % R] + list(sbar[1:]), zw))
    assert not _verify(d, srs, oracle, evals=(abar, sbar, (zw + 1) % R))
    # the evaluations of the PLAIN polynomials are not those of the committed ones
    assert not _verify(d, srs, oracle, evals=LO.evaluations(c, plain, ZETA))
    # a chunk blinder used in the [T~_c] but not in r~: the proof is that of another r~
    other = BO.Blinders(bl.b, bl.c, [(x + 1) % R for x in bl.d])
    d2 = BO.proof_case(c, z, log_ext, other, ALPHA, BETA, GAMMA, ZETA, V, SECRET)
    assert d2["t_s"] != d["t_s"] and d2["w"] != d["w"] and _verify(d2, srs, oracle)
    assert not _verify(d, srs, oracle, t_s=d2["t_s"])
    assert not _verify(d, srs, oracle, w=(d["w"] + 1) % R)


# ---- the library: what needs no device -------------------------------------------------------------------------------------------
def test_blinders_are_below_r_and_fresh():
    for t, log_ext in ((2, 2), (3, 2), (7, 3)):
        a, b = K.circuit_blinders(t, log_ext), K.circuit_blinders(t, log_ext)
        assert a.shape == (2 * t + 3 + (1 << log_ext) - 2, 4) and a.dtype == np.uint64
        for row in list(a) + list(b):
            assert sum(int(x) << (64 * i) for i, x in enumerate(row)) < R
        assert not np.array_equal(a, b)
        assert len({bytes(row) for row in np.concatenate([a, b])}) == 2 * a.shape[0]
    lib = K.load_library()
    out = np.zeros((32, 4), dtype=np.uint64)
    bad = K.KZG_ERR_INVALID_ARG
    assert lib.kzg_circuit_blinders(3, 2, None) == bad
    for t, log_ext in ((1, 2), (8, 3), (3, 1), (2, 4), (7, 2)):
        assert lib.kzg_circuit_blinders(t, log_ext, out.ctypes.data) == bad, (t, log_ext)
    assert not out.any()


def test_the_shape_rule():
    assert K.circuit_blinded_sizes(8, 3, 2) == (2 * 3 + 3 + 2, 3 * 8 + 3 + 3)
    assert K.circuit_blinded_sizes(16, 2, 2) == (9, 3 * 16 + 5)
    assert K.circuit_blinded_sizes(16, 7, 3) == (23, 7 * 16 + 10)
    assert K.circuit_blinded_sizes(1, 2, 3) == (13, 7 + 5)  # N = 8 = t n + t + 4
    for n, t, log_ext in ((4, 3, 2), (8, 7, 3), (1, 3, 2), (2, 3, 2), (1, 2, 2), (12, 3, 2), (8, 3, 1), (8, 1, 2), (8, 3, 4)):
        with pytest.raises(K.KzgError) as ei:
            K.circuit_blinded_sizes(n, t, log_ext)
        assert ei.value.status == K.KZG_ERR_INVALID_ARG, (n, t, log_ext)
    lib = K.load_library()
    assert lib.kzg_circuit_blinded_sizes(8, 3, 2, None, None) == K.KZG_OK


def test_null_context_and_null_pointers_are_refused():
    lib = K.load_library()
    a = np.zeros((64, 4), dtype=np.uint64)
    p = a.ctypes.data
    bad = K.KZG_ERR_INVALID_ARG
    # ctx, circuit, wires, stride, z, PI, three challenges, blinders, out_coeffs, out_p1s
    quot = [p, p, p, 8, p, None, p, p, p, p, p, p]
    # ctx, circuit, wires, stride, z, PI, T, five challenges, blinders, evals, proof
    opened = [p, p, p, 8, p, None, p, p, p, p, p, p, p, p, p]
    blind = [p, p, 8, 1, 8, p, 2, p, 10]  # ctx, evals, n, k, stride, blinders, nb, out, out_stride
    commit = blind[:7] + [p]
    calls = ((lib.kzg_circuit_quotient_blinded, quot, (3, 5, 10, 11)), (lib.kzg_circuit_quotient_blinded_device, quot, (3, 5, 11)),
             (lib.kzg_circuit_open_blinded, opened, (3, 5)), (lib.kzg_circuit_open_blinded_device, opened, (3, 5)),
             (lib.kzg_blind_evaluations, blind, (2, 3, 4, 6, 8)), (lib.kzg_commit_evaluations_blinded, commit, (2, 3, 4, 6)))
    # a context that is never read: the pointers are checked first (only the first word, "not a multi-device context", is looked at)
    ctx = np.zeros(1 << 16, dtype=np.uint8).ctypes.data
    for fn, args, optional in calls:
        assert fn(*([None] + args[1:])) == bad, fn.__name__
        for pos in range(1, len(args)):
            if pos in optional:  # sizes; pointers that may be NULL
                continue
            assert fn(*([ctx] + args[1:pos] + [None] + args[pos + 1:])) == bad, (fn.__name__, pos)


# ---- header, wrapper and library agree -----------------------------------------------------------------------------------------
def test_abi_exports_the_new_symbols():
    lib = K.load_library()
    header = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    hpp = open(os.path.join(ROOT, "include", "kzg_mi355x.hpp")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in K.ABI_SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, header), name
    for name in ("kzg_circuit_blinders", "kzg_commit_evaluations_blinded", "kzg_circuit_quotient_blinded", "kzg_circuit_open_blinded"):
        assert name + "(" in hpp, name
    for name in ("blinders", "quotient_blinded", "quotient_blinded_device", "open_blinded", "open_blinded_device"):
        assert callable(getattr(K.Circuit, name)), name
    for name in ("blind_evaluations_limbs", "commit_evaluations_blinded"):
        assert callable(getattr(K.Engine, name)), name
    assert callable(K.circuit_blinders) and "circuit_blinders" in K.__all__
    section = header[header.index("zero-knowledge circuit proofs"):header.index("int kzg_circuit_blinded_sizes(")]
    assert "SHAPE RULE" in section and "BLINDER ARRAY" in section and "L_T" in section
