"""CPU: the last round of a circuit's proof -- tests/linearise_oracle.py against itself, kzg_circuit_verify
on proofs made from the known secret (commitments [P(s)]G and the proof [h(s)]G: no GPU), its argument errors, the accumulation of
k_lin_combine (csrc/linearise_kernels.hip) replayed on the host at the magnitudes its bound comment allows
(tests/host/lin_reach_host.cpp: a stand-alone program built with g++, nothing is loaded into this process), the errors of the
device-side calls that are answered before any device is touched, and the export of every new symbol."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import circuit_oracle as CO
import fr_extremes as FE
import kzg_poly_commit_exploration_amd as K
import linearise_oracle as LO
import ntt_oracle as NO
import open_sets_oracle as SO
import perm_quotient_oracle as PQ
import trapdoor_oracle as TO

R = PQ.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA, BETA, GAMMA = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % R, 0x1F2E3D4C5B6A79881F2E3D4C5B6A7988 % R, 0x123456789ABCDEF0FEDCBA9876543210 % R
ZETA, V = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R, 0x6A09E667F3BCC908B2FB1366EA957D3E3ADEC17512775099DA2F590B0667322A % R
SECRET = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % R
NEW_SYMBOLS = ("kzg_circuit_open", "kzg_circuit_open_device", "kzg_circuit_linearise", "kzg_circuit_verify")

_CACHE = {}


def _case(k, t, log_ext, with_pi=True):
    """a satisfied circuit with its z, T and coefficient vectors, computed once"""
    key = (k, t, log_ext, with_pi)
    if key not in _CACHE:
        c = CO.satisfied(k, t, 300 + 10 * k + t, with_pi)
        z, last = CO.z_of(c, BETA, GAMMA)
        assert last == 1
        _CACHE[key] = (c, z, CO.quotient(c, z, ALPHA, BETA, GAMMA), LO.coefficients(c, z))
    return _CACHE[key]


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_pi", [True, False])
@pytest.mark.parametrize("k,t,log_ext", [(0, 3, 2), (1, 3, 2), (3, 3, 2), (4, 2, 2), (5, 3, 2), (2, 7, 3), (3, 2, 2)])
def test_the_linearisation_vanishes_at_zeta_exactly_for_the_true_quotient(k, t, log_ext, with_pi):
    c, z, T, coefs = _case(k, t, log_ext, with_pi)
    n = c.n
    w = NO.domain_root(k)
    rnd = random.Random(31 * k + t)
    for zeta in (rnd.randrange(R), ZETA, 1, w):
        r = LO.linearisation(c, coefs, T, log_ext, ALPHA, BETA, GAMMA, zeta)
        assert len(r) == n and PQ.horner(r, zeta) == 0, zeta
        assert LO.l0_at(n, zeta) == (1 if zeta == 1 else 0 if pow(zeta, n, R) == 1 else
                                     (pow(zeta, n, R) - 1) * pow(n * (zeta - 1), -1, R) % R)
        polys, set_of, sets, ys = LO.stack(c, coefs, r, zeta)
        assert len(polys) == 2 * t + 1 and set_of == [0] * (2 * t) + [1] and sets == [[zeta], [zeta * w % R]]
        assert SO.values(polys, set_of, sets) == ys and ys[0] == [0]
    zeta = ZETA
    # one coefficient of T changed
    bad = LO.chunks(T, n, log_ext)
    bad[0][0] = (bad[0][0] + 1) % R
    flat = [v for ch in bad for v in ch]
    assert PQ.horner(LO.linearisation(c, coefs, flat, log_ext, ALPHA, BETA, GAMMA, zeta), zeta) != 0
    # one wire value changed (T and z stay)
    wires = [list(col) for col in c.wires]
    wires[t - 1][n - 1] = (wires[t - 1][n - 1] + 1) % R
    other = CO.Circuit(c.ks, wires, c.sigmas, c.q_lin, c.q_mul, c.q_const, c.pi)
    assert PQ.horner(LO.linearisation(other, LO.coefficients(other, z), T, log_ext, ALPHA, BETA, GAMMA, zeta), zeta) != 0
    # one public input changed
    if with_pi:
        pi = list(c.pi)
        pi[0] = (pi[0] + 1) % R
        other = CO.Circuit(c.ks, c.wires, c.sigmas, c.q_lin, c.q_mul, c.q_const, pi)
        assert PQ.horner(LO.linearisation(other, LO.coefficients(other, z), T, log_ext, ALPHA, BETA, GAMMA, zeta), zeta) != 0


def test_public_inputs_by_lagrange_polynomials_agree_with_the_interpolant():
    c, z, T, coefs = _case(3, 3, 2)
    for zeta in (ZETA, 1, NO.domain_root(3), pow(NO.domain_root(3), 3, R)):
        assert LO.public_input_at(c.n, c.pi, zeta) == PQ.horner(coefs[3], zeta)
        assert LO.public_input_at(c.n, c.pi[:7], zeta) == PQ.horner(NO.intt(c.pi[:7] + [0]), zeta)


# ---- the verifier on proofs made from the secret -------------------------------------------------------------------------------
def _point(oracle, v):
    return K.G1Point(oracle.p1_mult(oracle.p1_generator(), v % R))


@pytest.fixture(scope="module")
def srs(oracle):
    """[s^j]G1 for j < 2 and [s^j]G2 for j <= 2"""
    g1 = np.stack([oracle.p1_mult(oracle.p1_generator(), pow(SECRET, j, R)) for j in range(2)])
    g2 = np.stack([K.srs_g2_at(TO.secret_be(SECRET), j) for j in range(3)])
    return g1, g2


def _proof_case(oracle, k, t, log_ext, zeta=ZETA):
    c, z, T, coefs = _case(k, t, log_ext)
    key, wires, zc, _ = coefs
    r = LO.linearisation(c, coefs, T, log_ext, ALPHA, BETA, GAMMA, zeta)
    polys, set_of, sets, ys = LO.stack(c, coefs, r, zeta)
    last = max(i for i, p in enumerate(c.pi) if p)
    d = dict(c=c, coefs=coefs, log_ext=log_ext, zeta=zeta, v=V, evals=LO.evaluations(c, coefs, zeta), public=list(c.pi[:last + 1]),
             key_s=[PQ.horner(col, SECRET) for col in key], wire_s=[PQ.horner(col, SECRET) for col in wires],
             z_s=PQ.horner(zc, SECRET), t_s=[PQ.horner(ch, SECRET) for ch in LO.chunks(T, c.n, log_ext)],
             w=SO.proof_scalar(polys, set_of, sets, V, SECRET))
    # the verifier's combination is the commitment of r, and the stack satisfies the verifier's equation
    rs = LO.r_scalar(c, coefs, log_ext, ALPHA, BETA, GAMMA, zeta, d["evals"], d["public"], d["key_s"], d["z_s"], d["t_s"])
    assert rs == PQ.horner(r, SECRET)
    sides, b_t = SO.verifier_sides([rs] + d["wire_s"] + d["key_s"][t + 2:2 * t + 1] + [d["z_s"]], set_of, sets, ys, V, SECRET)
    assert sum(a * b for a, b in sides) % R == d["w"] * b_t % R
    return d


def _verify(d, srs, oracle, **changes):
    d = dict(d, **changes)
    c = d["c"]
    pts = lambda scalars: [_point(oracle, s) for s in scalars]
    abar, sbar, zw = d["evals"]
    ev = ([K.Scalar(a) for a in abar], [K.Scalar(s) for s in sbar], K.Scalar(zw))
    return K.circuit_verify(pts(d["key_s"]), c.n, d["log_ext"], [K.Scalar(k) for k in c.ks], pts(d["wire_s"]), _point(oracle, d["z_s"]),
                            pts(d["t_s"]), [K.Scalar(p) for p in d["public"]], ev, K.Scalar(d.get("alpha", ALPHA)), K.Scalar(BETA),
                            K.Scalar(GAMMA), K.Scalar(d["zeta"]), K.Scalar(d["v"]), _point(oracle, d["w"]), srs[0], srs[1])


@pytest.mark.parametrize("k,t,log_ext", [(0, 3, 2), (1, 3, 2), (3, 3, 2), (2, 2, 2), (2, 7, 3)])
def test_verify_accepts_and_rejects(oracle, srs, k, t, log_ext):
    d = _proof_case(oracle, k, t, log_ext)
    assert _verify(d, srs, oracle)
    # the whole column of public inputs is the same statement as its rows up to the last non-zero one
    assert _verify(d, srs, oracle, public=list(d["c"].pi))
    abar, sbar, zw = d["evals"]
    for j in sorted({0, t - 1}):  # one evaluation
        bad = list(abar)
        bad[j] = (bad[j] + 1) % R
        assert not _verify(d, srs, oracle, evals=(bad, sbar, zw)), j
    assert not _verify(d, srs, oracle, evals=(abar, [(sbar[0] + 1) % R] + list(sbar[1:]), zw))
    assert not _verify(d, srs, oracle, evals=(abar, sbar, (zw + 1) % R))
    # two commitments of T's chunks swapped (for n = 1 the quotient of this circuit is zero and so is every chunk: nothing to swap)
    ts = list(d["t_s"])
    if ts[0] != ts[1]:
        ts[0], ts[1] = ts[1], ts[0]
        assert not _verify(d, srs, oracle, t_s=ts)
    else:
        assert d["c"].n == 1
    pub = list(d["public"])  # one public input
    pub[0] = (pub[0] + 1) % R
    assert not _verify(d, srs, oracle, public=pub)
    assert d["public"][-1] != 0 and not _verify(d, srs, oracle, public=d["public"][:-1])  # n_public shortened past a non-zero row
    # v and zeta.  For n = 1 every polynomial of the stack is a constant: the evaluations are those at ANY point, the linearisation
    # at zeta + 1 of the true T vanishes there too, and h = 0 under any v -- the altered statements are true, and accepted
    single = d["c"].n == 1
    assert (d["w"] == 0) == single
    assert _verify(d, srs, oracle, v=(V + 1) % R) == single
    assert _verify(d, srs, oracle, zeta=(ZETA + 1) % R) == single
    assert not _verify(d, srs, oracle, alpha=(ALPHA + 1) % R)
    for j in (0, t + 1, 2 * t + 1):  # one commitment of the key: a selector, q_C, the last sigma
        ks = list(d["key_s"])
        ks[j] = (ks[j] + 1) % R
        assert not _verify(d, srs, oracle, key_s=ks), j
    assert not _verify(d, srs, oracle, w=(d["w"] + 1) % R)  # the proof


@pytest.mark.parametrize("which", ["one", "root"])
def test_verify_with_zeta_inside_the_domain(oracle, srs, which):
    zeta = 1 if which == "one" else NO.domain_root(3)
    d = _proof_case(oracle, 3, 3, 2, zeta=zeta)
    assert _verify(d, srs, oracle)
    abar, sbar, zw = d["evals"]
    assert not _verify(d, srs, oracle, evals=(abar, sbar, (zw + 1) % R))
    pub = list(d["public"])
    pub[0 if which == "one" else 1] += 1  # the row zeta sits on (row 1 holds no public input in this circuit, and now does)
    assert not _verify(d, srs, oracle, public=pub)


def test_verifier_argument_errors(oracle, srs):
    lib = K.load_library()
    k, t, log_ext = 2, 3, 2
    d = _proof_case(oracle, k, t, log_ext)
    c = d["c"]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rows = lambda v: np.ascontiguousarray(np.stack([K.Scalar(x).limbs() for x in v]), dtype=np.uint64)
    pts = lambda v: np.ascontiguousarray(np.stack([_point(oracle, x).p1 for x in v]), dtype=np.uint64)
    not_fr = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    abar, sbar, zw = d["evals"]
    base = dict(key=pts(d["key_s"]), n=c.n, t=t, log_ext=log_ext, shifts=rows(c.ks), wires=pts(d["wire_s"]), z=pts([d["z_s"]]),
                ts=pts(d["t_s"]), public=rows(d["public"]), n_public=len(d["public"]), evals=rows(list(abar) + list(sbar) + [zw]),
                alpha=rows([ALPHA]), beta=rows([BETA]), gamma=rows([GAMMA]), zeta=rows([ZETA]), v=rows([V]), proof=pts([d["w"]]),
                g1=np.ascontiguousarray(srs[0]), g2=np.ascontiguousarray(srs[1]))
    order = ["key", "n", "t", "log_ext", "shifts", "wires", "z", "ts", "public", "n_public", "evals", "alpha", "beta", "gamma", "zeta",
             "v", "proof", "g1", None, "g2", None]
    ok = C.c_int(0)

    def call(null=None, valid=C.byref(ok), **changes):
        a = dict(base, **changes)
        args = []
        for pos, name in enumerate(order):
            if name is None:
                args.append(144 if pos == 18 else 288)
            elif name == null:
                args.append(None)
            else:
                args.append(a[name] if isinstance(a[name], int) else p(a[name]))
        return lib.kzg_circuit_verify(*args, valid)

    bad = K.KZG_ERR_INVALID_ARG
    assert call() == K.KZG_OK and ok.value == 1
    for name in order:
        if name is not None and not isinstance(base[name], int):
            assert call(null=name) == bad, name
    assert call(valid=None) == bad
    assert call(public=base["public"], n_public=0, null="public") == K.KZG_OK and ok.value == 0  # no public inputs: legal, another statement
    assert call(t=1) == bad and call(t=K.KZG_PQ_MAX_COLUMNS + 1) == bad
    assert call(log_ext=1) == bad and call(log_ext=K.KZG_PQ_MAX_LOG_EXT + 1) == bad  # t + 1 > e; e too large
    assert call(n=3) == bad and call(n=0) == bad
    assert call(n_public=c.n + 1) == bad
    for name, row in (("alpha", 0), ("beta", 0), ("gamma", 0), ("zeta", 0), ("v", 0), ("evals", 2 * t - 1), ("evals", 0), ("public", 0),
                      ("shifts", t - 1)):
        a = base[name].copy()
        a[row] = not_fr
        assert call(**{name: a}) == bad, name
    for name, row in (("key", 0), ("key", 2 * t + 1), ("key", t + 2), ("wires", t - 1), ("z", 0), ("ts", 1), ("proof", 0)):
        a = base[name].copy()
        a[row, 0] ^= 1
        assert call(**{name: a}) == bad, (name, row)
    off_twist = base["g2"].copy()
    off_twist[1, 0] ^= 1
    assert call(g2=off_twist) == bad
    assert call() == K.KZG_OK and ok.value == 1


# ---- the device-side calls: what is answered before any device is touched --------------------------------------------------------
def test_null_context_and_null_pointers_are_refused():
    lib = K.load_library()
    a = np.zeros((64, 4), dtype=np.uint64)
    p = a.ctypes.data
    bad = K.KZG_ERR_INVALID_ARG
    opened = [p, p, p, 4, p, None, p, p, p, p, p, p, p, p]  # ctx, circuit, wires, stride, z, PI, T, five challenges, evals, proof
    lin = opened[:11] + [p, p]                              # ... four challenges, evals, r
    assert lib.kzg_circuit_open(*([None] + opened[1:])) == bad
    assert lib.kzg_circuit_open_device(*([None] + opened[1:])) == bad
    assert lib.kzg_circuit_linearise(*([None] + lin[1:])) == bad
    # a context that is never read: the pointers are checked first (only the first word, "not a multi-device context", is looked at)
    ctx = np.zeros(1 << 16, dtype=np.uint8).ctypes.data
    for fn, args in ((lib.kzg_circuit_open, opened), (lib.kzg_circuit_open_device, opened), (lib.kzg_circuit_linearise, lin)):
        for pos in range(1, len(args)):
            if pos in (3, 5):  # the stride; PI may be NULL
                continue
            assert fn(*([ctx] + args[1:pos] + [None] + args[pos + 1:])) == bad, (fn.__name__, pos)


# ---- header, wrapper and library agree -----------------------------------------------------------------------------------------
def test_abi_exports_the_new_symbols():
    lib = K.load_library()
    header = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in K.ABI_SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, header), name
    for name in ("open", "open_device", "linearise"):
        assert callable(getattr(K.Circuit, name)), name
    assert callable(K.circuit_verify) and "circuit_verify" in K.__all__
    assert "#define KZG_ABI_VERSION 4" in header and K.KZG_ABI_VERSION == 4
    section = header[header.index("a circuit's proof, last round"):header.index("int kzg_circuit_open(")]
    assert "SOUNDNESS" in section and "Nothing is hashed here" in section and "gate_coset" in section
    hpp = open(os.path.join(ROOT, "include", "kzg_mi355x.hpp")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in hpp, name


# ---- the kernel's accumulation at its bounds -----------------------------------------------------------------------------------
# fr30.hip.h, fr30_mac: the raw sum of a normalised value and one product stays within 2^30 + 4, a carry pass returns digits within
# 2^29 + 4, and k_lin_combine's bound comment: at most kLinMaxColumns = 32 products below 0.5001 r + r / 2^14 and one canonical
# constant, so an accumulator stays below 17.1 r; fr30_sum_reduce returns below 0.51 r; a column of a product stays inside the
# signed 64-bit accumulator.
COLUMNS = 32
RAW_BOUND = (1 << 30) + 4
NORM_BOUND = (1 << 29) + 4


def _top(c):
    """|digit 8| of a value below c r in magnitude with balanced lower digits: c r / 2^240 rounded up, plus the half digit"""
    return (int(c * 10000) * 0x73EE + 9999) // 10000 + 1


ACC_TOP, PRODUCT_TOP, REDUCED_TOP, COLUMN_BOUND = _top(17.1), _top(0.5002), _top(0.51), 1 << 63
INV256 = pow(FE.R256, -1, R)


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lin") / "lin_reach")
    # -fwrapv: a digit sum that overflowed would wrap on the device, and so must it here
    subprocess.run(["g++", "-O2", "-fwrapv", "-o", exe, os.path.join(ROOT, "tests", "host", "lin_reach_host.cpp")], check=True)

    def run(lines):
        """lines: [(konst image, [(plain multiplier, coefficient image)])] -> (report, the results as plain values)"""
        hx = lambda v: "%064x" % v
        text = "%d %d\n" % (len(lines), len(lines[0][1]))
        for konst, pairs in lines:
            text += " ".join([hx(konst)] + [hx(m % R * FE.R256 % R) + " " + hx(c) for m, c in pairs]) + "\n"
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == 6 + len(lines)
        return [int(v) for v in out[:6]], [int(v, 16) * INV256 % R for v in out[6:]]

    return run


def _want(konst, pairs):
    return (konst + sum(m * c for m, c in pairs)) * INV256 % R


@pytest.mark.parametrize("sign", [1, -1])
def test_replay_thirty_two_aligned_products_and_the_constant(replay, sign):
    """every product just inside +r/2 (or every one just inside -r/2) whatever the multiplier, the constant pushed the same way:
    |acc| at its extreme.  Just inside: a product comes back within r / 2^14 of its centred residue, so a term AT r/2 could land
    on either side; 2^242 keeps every one on its own"""
    h = FE.H_PLUS - (1 << 242) if sign > 0 else FE.H_MINUS + (1 << 242)
    mults = FE.extremal_multipliers() + [1, R - 1, ALPHA, BETA]
    rnd = random.Random(5 + sign)
    lines = []
    for i in range(24):
        ms = [mults[(i + 3 * j) % len(mults)] if (i + j) % 5 else rnd.randrange(1, R) for j in range(COLUMNS)]
        lines.append((R - 1 if sign > 0 else 0, list(zip(ms, FE.compensated(ms, h)))))
    rep, got = replay(lines)
    print("sign %d: raw %d norm %d acc top %d product top %d reduced top %d column 2^%.2f" % (
        sign, rep[0], rep[1], rep[2], rep[3], rep[4], np.log2(float(rep[5]))))
    assert rep[0] <= RAW_BOUND and rep[1] <= NORM_BOUND and rep[2] <= ACC_TOP < (1 << 22), rep
    assert rep[3] <= PRODUCT_TOP and rep[4] <= REDUCED_TOP and rep[5] < COLUMN_BOUND, rep
    assert rep[2] >= int(0.49 * COLUMNS * 0x73ED), rep  # the extreme was reached: within 2 % of 32 r / 2
    assert got == [_want(k, pairs) for k, pairs in lines]


def test_replay_digit_extremal_coefficients_and_multipliers(replay):
    """half values and digit-extremal images in every coefficient position against extremal and ordinary multipliers"""
    images = FE.half_values() + FE.digit_extremal() + [1, R - 1, FE.R256, 0]
    mults = FE.extremal_multipliers() + [1, R - 1, 0]
    rnd = random.Random(77)
    lines = []
    for i in range(len(images)):
        pairs = [(mults[(i + j) % len(mults)] if j % 3 else rnd.randrange(R), images[(i + 5 * j) % len(images)]) for j in range(COLUMNS)]
        lines.append((images[(7 * i) % len(images)], pairs))
    rep, got = replay(lines)
    print("extremal: raw %d norm %d acc top %d product top %d reduced top %d column 2^%.2f" % (
        rep[0], rep[1], rep[2], rep[3], rep[4], np.log2(float(rep[5]))))
    assert rep[0] <= RAW_BOUND and rep[1] <= NORM_BOUND and rep[2] <= ACC_TOP, rep
    assert rep[3] <= PRODUCT_TOP and rep[4] <= REDUCED_TOP and rep[5] < COLUMN_BOUND, rep
    assert got == [_want(k, pairs) for k, pairs in lines]
