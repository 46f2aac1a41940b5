"""CPU: tests/circuit_oracle.py against itself, the arithmetic of k_ck_constraints (csrc/circuit_kernels.hip) replayed on the host
at the magnitudes its bound comment allows (tests/host/ck_reach_host.cpp: a stand-alone program built with g++, nothing is loaded
into this process), and the argument errors that need no GPU."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import circuit_oracle as CO
import fr_extremes as FE
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import perm_quotient_oracle as PQ

R = PQ.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA, BETA, GAMMA = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % R, 0x1F2E3D4C5B6A79881F2E3D4C5B6A7988 % R, 0x123456789ABCDEF0FEDCBA9876543210 % R


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_pi", [True, False])
@pytest.mark.parametrize("t", [2, 3])
@pytest.mark.parametrize("k", [0, 1, 2, 5])
def test_satisfied_circuits_divide_exactly(k, t, with_pi):
    n = 1 << k
    c = CO.satisfied(k, t, 100 * k + t, with_pi)
    z, last = CO.z_of(c, BETA, GAMMA)
    assert last == 1
    gate = CO.gate_coeffs(c)
    assert len(gate) <= 3 * (n - 1) + 1
    assert [PQ.horner(gate, x) for x in GO.domain(k)] == [0] * n  # the gate vanishes on H
    assert CO.remainder(c, z, ALPHA, BETA, GAMMA) == []
    T = CO.quotient(c, z, ALPHA, BETA, GAMMA)
    assert T == PQ.divide_vanishing(CO.numerator(c, z, ALPHA, BETA, GAMMA), n)[0]
    fc, zc = [NO.intt(col) for col in c.wires], NO.intt(z)
    rnd = random.Random(k + t)
    for _ in range(2):
        zeta = rnd.randrange(R)
        assert CO.check_at(zeta, T, c, fc, zc, ALPHA, BETA, GAMMA)  # agrees with the division
        if T:
            bad = list(T)
            bad[-1] = (bad[-1] + 1) % R
            assert not CO.check_at(zeta, bad, c, fc, zc, ALPHA, BETA, GAMMA)
    # the gate really is in T: without it the permutation's own quotient differs
    if k >= 1:
        assert T != PQ.quotient(c.wires, c.sigmas, z, c.ks, ALPHA, BETA, GAMMA)


@pytest.mark.parametrize("k", [1, 2, 5])
def test_a_perturbed_gate_row_or_a_broken_copy_does_not_divide(k):
    n, t = 1 << k, 3
    c = CO.satisfied(k, t, 7 * k + t)
    z, _ = CO.z_of(c, BETA, GAMMA)
    bad = CO.Circuit(c.ks, c.wires, c.sigmas, c.q_lin, c.q_mul, [(v + (1 if i == n - 1 else 0)) % R for i, v in enumerate(c.q_const)], c.pi)
    assert CO.gate_rows(bad) == [0] * (n - 1) + [1]
    assert CO.remainder(bad, z, ALPHA, BETA, GAMMA) != []
    ident = GO.identity_sigmas(k, c.ks)
    j, i = [(j, i) for j in range(t) for i in range(n) if c.sigmas[j][i] != ident[j][i]][-1]
    bw = [list(col) for col in c.wires]
    bw[j][i] = (bw[j][i] + 1) % R
    assert CO.remainder(c, z, ALPHA, BETA, GAMMA, wires=bw) != []
    assert CO.remainder(c, [v * 5 % R for v in z], ALPHA, BETA, GAMMA) != []


def test_a_term_that_is_a_multiple_of_the_vanishing_polynomial_adds_its_cofactor():
    k, t = 3, 2
    n = 1 << k
    c = CO.satisfied(k, t, 31)
    z, _ = CO.z_of(c, BETA, GAMMA)
    rnd = random.Random(k)
    Rc = [rnd.randrange(R) for _ in range(n)]
    extra = [((Rc[i - n] if n <= i < 2 * n else 0) - (Rc[i] if i < n else 0)) % R for i in range(2 * n)]  # Z_H R
    T0, T1 = CO.quotient(c, z, ALPHA, BETA, GAMMA), CO.quotient(c, z, ALPHA, BETA, GAMMA, extra=extra)
    width = max(len(T0), len(T1), n)
    pad = lambda v: list(v) + [0] * (width - len(v))
    assert pad(T1) == [(a + b) % R for a, b in zip(pad(T0), pad(Rc))]
    assert CO.check_at(12345, T1, c, [NO.intt(col) for col in c.wires], NO.intt(z), ALPHA, BETA, GAMMA, extra=extra)


# ---- the kernel's arithmetic at its bounds -------------------------------------------------------------------------------------
# The bounds the unit's header states (circuit_kernels.hip, "Bounds"), per quantity, in the order the replay reports them:
# f + gamma, the factors a_j / b_j, D = A - B, z - one, P (the gate's products), S.
NORM = (1 << 29) + 4                 # |digit 0..7| of a load or a carry pass (fr30.hip.h); a product stays below 2^29
RAW_BOUNDS = [2 * NORM,              # f + gamma: two normalised values
              NORM + (1 << 29),      # a normalised value plus one product: 2^30 + 4
              1 << 30,               # the difference of two products
              2 * NORM,              # z - one: two normalised values
              NORM + (1 << 29),      # P: a normalised value plus one product, one product per carry pass
              2 * NORM]              # S: a normalised value plus one product or one canonical value


def _top(c):
    """|digit 8| of a value below c r in magnitude with balanced lower digits: c r / 2^240 rounded up, plus the half digit"""
    return (int(c * 10000) * 0x73EE + 9999) // 10000 + 1


TOP_BOUNDS = [_top(2), _top(2.51), _top(1.0004), _top(1), _top(4.002), _top(4.501)]
PRODUCT_TOP = _top(0.5004)           # every product: the last one, S zinv, is below 0.5001 r + 4.501 r^2 / 2^270 < 0.5004 r
COLUMN_BOUND = 1 << 62               # the header: a column of the product with S stays below 2^62, inside the 64-bit accumulator
INV256 = pow(FE.R256, -1, R)
INV242 = pow(1 << 242, -1, R)


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ck") / "ck_reach")
    # -fwrapv: a digit sum that overflowed would wrap on the device, and so must it here
    subprocess.run(["g++", "-O2", "-fwrapv", "-o", exe, os.path.join(ROOT, "tests", "host", "ck_reach_host.cpp")], check=True)

    def run(t, alpha, beta, gamma, ks, lines, has_pi, has_gate):
        """lines: plain values [w, zinv, z, zrot, l0, qc, pi, gate, qm, f_0.., s_0.., q_0..].  Returns (report, results)"""
        img = lambda v: "%064x" % (v % R * FE.R256 % R)
        head = " ".join(img(v) for v in [alpha, beta, gamma] + [beta * k * 7 for k in ks])
        text = "%d %d %d %d\n%s\n" % (t, len(lines), 1 if has_pi else 0, 1 if has_gate else 0, head) + \
               "".join(" ".join(img(v) for v in l) + "\n" for l in lines)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == 15 + len(lines)
        return [int(v) for v in out[:15]], [int(v, 16) * INV256 % R for v in out[15:]]

    return run


def _want(t, alpha, beta, gamma, ks, l, has_pi, has_gate):
    w, zinv, z, zr, l0, qc, pi, gate, qm = l[:9]
    f, s, q = l[9:9 + t], l[9 + t:9 + 2 * t], l[9 + 2 * t:9 + 3 * t]
    a, b = z, zr
    for j in range(t):
        a = a * ((f[j] + beta * ks[j] * 7 % R * w + gamma) % R) % R
        b = b * ((f[j] + beta * s[j] + gamma) % R) % R
    g = (sum(q[j] * f[j] for j in range(t)) + qm * f[0] * f[1] + qc + (pi if has_pi else 0) + (gate if has_gate else 0)) % R
    return (g + alpha * (a - b) + alpha * alpha % R * (z - 1) % R * l0) % R * zinv % R


def _lines(t, aligned):
    """64 points: half values and digit-extremal images in every data position, extremal twiddles and vanishing inverses.
    aligned = +1 / -1: the selectors are chosen so that EVERY product of the gate, as the lazy value fr30_mul returns (the centred
    residue of x y 2^242), sits at +r/2 or at -r/2: all t + 1 signs aligned, |P| at its extreme"""
    images = [v * INV256 % R for v in FE.half_values() + FE.digit_extremal() + [1, R - 1, FE.R256, 0]]
    mults = FE.extremal_multipliers() + [1, R - 1]
    rnd = random.Random(1000 * t + aligned)
    target = {1: (R - 1) // 2, -1: (R + 1) // 2}.get(aligned)
    lines = []
    for i in range(64):
        l = [mults[i % len(mults)], mults[(i // len(mults) + 3 * i) % len(mults)]]
        l += [images[(5 * i + 3 * c) % len(images)] if i % 4 else rnd.randrange(R) for c in range(7 + 3 * t)]
        if aligned:
            f = l[9:9 + t]
            for j in range(t):
                if f[j] % R == 0:
                    f[j] = l[9 + j] = 1 + rnd.randrange(R - 1)
            for j in range(t):  # image(q) image(f) / 2^270 = q f 2^242 = target
                l[9 + 2 * t + j] = target * pow(f[j] * (1 << 242) % R, -1, R) % R
            l[8] = target * pow(f[0] * f[1] % R * (1 << 242) % R, -1, R) % R  # image(q_M) image(f_0 f_1) / 2^270
            l[5] = l[6] = l[7] = (R - 1) if aligned > 0 else 0  # q_C, PI, G': the canonical values pushed the same way
        lines.append(l)
    return lines


@pytest.mark.parametrize("alpha,beta", [(ALPHA, BETA), (0, BETA), (ALPHA, 0), (FE.extremal_multipliers()[0], FE.extremal_multipliers()[2])])
@pytest.mark.parametrize("aligned", [0, 1, -1])
@pytest.mark.parametrize("t", [2, 7])
def test_replay_extremal_images_twiddles_and_aligned_selectors(replay, t, aligned, alpha, beta):
    ks = GO.shifts(t)
    lines = _lines(t, aligned)
    for has_pi, has_gate in ((True, True), (False, False)):
        rep, got = replay(t, alpha, beta, GAMMA, ks, lines, has_pi, has_gate)
        print("t=%d aligned=%d pi=%d gate=%d raw %s top %s norm %d product top %d column 2^%.2f" % (
            t, aligned, has_pi, has_gate, rep[:6], rep[6:12], rep[12], rep[13], np.log2(float(rep[14]))))
        assert all(g <= bound for g, bound in zip(rep[:6], RAW_BOUNDS)), (rep[:6], RAW_BOUNDS)
        assert all(g <= bound for g, bound in zip(rep[6:12], TOP_BOUNDS)), (rep[6:12], TOP_BOUNDS)
        assert rep[12] <= NORM and rep[13] <= PRODUCT_TOP and rep[14] < COLUMN_BOUND, rep[12:]
        assert all(rep[:6]), rep  # every sum was seen
        if aligned:  # the extreme was reached: |P| within 2 % of (t + 1) r / 2
            assert rep[10] >= int(0.49 * (t + 1) * 0x73ED), (rep[10], t)
        assert got == [_want(t, alpha, beta, GAMMA, ks, l, has_pi, has_gate) for l in lines]


# ---- argument errors that need no GPU ------------------------------------------------------------------------------------------
def test_null_context_is_refused_by_every_entry_point():
    lib = K.load_library()
    a = np.zeros((64, 4), dtype=np.uint64)
    p = a.ctypes.data
    h = C.c_void_p(0xDEAD)
    assert lib.kzg_circuit_create(None, p, p, p, p, 4, 2, 4, p, 2, None, C.byref(h)) == K.KZG_ERR_INVALID_ARG
    assert h.value is None  # *out is NULL after a failed create
    assert lib.kzg_circuit_destroy(None, p) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_circuit_quotient(None, p, p, 4, p, None, p, p, p, None, p, None) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_circuit_quotient_device(None, p, p, 4, p, None, p, p, p, None, p) == K.KZG_ERR_INVALID_ARG
    ptr, ln = C.c_void_p(), C.c_size_t(0)
    assert lib.kzg_circuit_column_device(None, p, 0, 0, C.byref(ptr), C.byref(ln)) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_circuit_create(None, p, p, p, p, 4, 2, 4, p, 2, None, None) == K.KZG_ERR_INVALID_ARG


def test_constants_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    for name in ("KZG_CIRCUIT_MIN_COLUMNS", "KZG_CIRCUIT_COL_QLIN", "KZG_CIRCUIT_COL_QM", "KZG_CIRCUIT_COL_QC", "KZG_CIRCUIT_COL_SIGMA",
                 "KZG_CIRCUIT_COL_L0", "KZG_CIRCUIT_VALUES", "KZG_CIRCUIT_COEFFS", "KZG_CIRCUIT_COSET"):
        assert "#define %s %d\n" % (name, getattr(K, name)) in text, name
    assert K.KZG_CIRCUIT_MIN_COLUMNS == 2 and K.KZG_CIRCUIT_COL_QLIN + K.KZG_PQ_MAX_COLUMNS <= K.KZG_CIRCUIT_COL_QM
    assert K.KZG_CIRCUIT_COL_SIGMA + K.KZG_PQ_MAX_COLUMNS <= K.KZG_CIRCUIT_COL_L0
    assert "#define KZG_ABI_VERSION 4" in text
