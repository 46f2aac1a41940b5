"""CPU: tests/perm_quotient_oracle.py against itself, the arithmetic of k_pq_constraints (csrc/quotient_kernels.hip) replayed on
the host at the magnitudes its bound comment allows (tests/host/pq_reach_host.cpp: a stand-alone program built with g++, nothing
is loaded into this process), and the argument errors that need no GPU."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import fr_extremes as FE
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import perm_quotient_oracle as PQ

R = PQ.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA, BETA, GAMMA = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % R, 0x1F2E3D4C5B6A79881F2E3D4C5B6A7988 % R, 0x123456789ABCDEF0FEDCBA9876543210 % R


def _argument(k, t, seed):
    ks = GO.shifts(t)
    wires, sigmas = GO.true_permutation(k, t, ks, seed)
    z, last = PQ.z_of(wires, sigmas, ks, BETA, GAMMA)
    assert last == 1
    return ks, wires, sigmas, z


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_ext", [0, 1, 3])
@pytest.mark.parametrize("length", [1, 2, 3, 8])
def test_coset_extension_is_evaluation_at_the_coset_points(length, log_ext):
    rnd = random.Random(10 * length + log_ext)
    log_N = (length - 1).bit_length() + log_ext
    c = [rnd.randrange(R) for _ in range(length)]
    pts = PQ.coset_points(log_N)
    assert len(set(pts)) == 1 << log_N and pts[0] == 7 and all(pow(x, 1 << log_N, R) == pow(7, 1 << log_N, R) for x in pts)
    assert PQ.coset_extend(c, log_N) == PQ.coset_extend_direct(c, log_N)


@pytest.mark.parametrize("t", [1, 2, 3])
@pytest.mark.parametrize("k", [0, 1, 2, 5])
def test_true_permutations_divide_exactly(k, t):
    n = 1 << k
    ks, wires, sigmas, z = _argument(k, t, 100 * k + t)
    num = PQ.num_coeffs(wires, sigmas, z, ks, ALPHA, BETA, GAMMA)
    assert len(num) <= (n - 1) + t * max(n - 1, 1) + 1  # (t + 1)(n - 1); at n = 1 the factor beta k_j X still has degree one
    T, rem = PQ.divide_vanishing(num, n)
    assert rem == [] and T == PQ.quotient(wires, sigmas, z, ks, ALPHA, BETA, GAMMA)
    coeffs = lambda cols: [NO.intt(c) for c in cols]
    rnd = random.Random(k + t)
    for _ in range(2):
        zeta = rnd.randrange(R)
        assert PQ.check_at(zeta, T, coeffs(wires), coeffs(sigmas), NO.intt(z), n, ks, ALPHA, BETA, GAMMA)
        if T:
            bad = list(T)
            bad[-1] = (bad[-1] + 1) % R
            assert not PQ.check_at(zeta, bad, coeffs(wires), coeffs(sigmas), NO.intt(z), n, ks, ALPHA, BETA, GAMMA)
    # the coset route: Num / Z_H on the coset is T on the coset
    log_N = k + max(1, t.bit_length())
    ext = lambda cols: [PQ.coset_extend(NO.intt(c), log_N) for c in cols]
    got = PQ.constraints_on_coset(ext(wires), ext(sigmas), ext([z])[0], n, ks, ALPHA, BETA, GAMMA)
    assert got == PQ.coset_extend(T + [0] * (1 if not T else 0), log_N)


@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("k", [1, 2, 5])
def test_broken_arguments_do_not_divide(k, t):
    n = 1 << k
    ks, wires, sigmas, z = _argument(k, t, 7 * k + t)
    ident = GO.identity_sigmas(k, ks)
    moved = [(j, i) for j in range(t) for i in range(n) if sigmas[j][i] != ident[j][i]]
    j, i = moved[-1]
    bad = [list(c) for c in wires]
    bad[j][i] = (bad[j][i] + 1) % R
    assert PQ.divide_vanishing(PQ.num_coeffs(bad, sigmas, z, ks, ALPHA, BETA, GAMMA), n)[1] != []
    # z with last != 1: z c for c != 1 keeps the recurrence and breaks z_0 = 1 -- only the alpha^2 term notices
    zc = [v * 5 % R for v in z]
    assert PQ.divide_vanishing(PQ.num_coeffs(wires, sigmas, zc, ks, ALPHA, BETA, GAMMA), n)[1] != []
    # ... and a z whose recurrence closes on a value other than one
    bz, blast = PQ.z_of(bad, sigmas, ks, BETA, GAMMA)
    assert blast != 1 and PQ.divide_vanishing(PQ.num_coeffs(bad, sigmas, bz, ks, ALPHA, BETA, GAMMA), n)[1] != []


@pytest.mark.parametrize("k", [0, 2, 4])
def test_a_gate_term_that_is_a_multiple_of_the_vanishing_polynomial_adds_its_cofactor(k):
    n, t = 1 << k, 2
    ks, wires, sigmas, z = _argument(k, t, 31 + k)
    rnd = random.Random(k)
    Rc = [rnd.randrange(R) for _ in range(n + 1)]
    gate = [0] * (2 * n + 1)  # Z_H R
    for i, c in enumerate(Rc):
        gate[i + n] = (gate[i + n] + c) % R
        gate[i] = (gate[i] - c) % R
    T0 = PQ.quotient(wires, sigmas, z, ks, ALPHA, BETA, GAMMA)
    T1 = PQ.quotient(wires, sigmas, z, ks, ALPHA, BETA, GAMMA, gate)
    width = max(len(T0), len(T1), len(Rc))
    pad = lambda c: list(c) + [0] * (width - len(c))
    assert pad(T1) == [(a + b) % R for a, b in zip(pad(T0), pad(Rc))]


# ---- the kernel's arithmetic at its bounds -------------------------------------------------------------------------------------
# The bounds the unit's header states (quotient_kernels.hip, "Bounds"), per quantity, in the order the replay reports them:
# f + gamma, the factors a_j / b_j, D = A - B, z - one, S.
NORM = (1 << 29) + 4                 # |digit 0..7| of a load or a carry pass (fr30.hip.h); a product stays below 2^29
RAW_BOUNDS = [2 * NORM,              # f + gamma: two normalised values
              NORM + (1 << 29),      # a normalised value plus one product: 2^30 + 4
              1 << 30,               # the difference of two products
              2 * NORM,              # z - one: two normalised values
              NORM + (1 << 29)]      # S: a normalised value plus one product, one product per carry pass


def _top(c):
    """|digit 8| of a value below c r in magnitude with balanced lower digits: c r / 2^240 rounded up, plus the half digit"""
    return (int(c * 10000) * 0x73EE + 9999) // 10000 + 1


TOP_BOUNDS = [_top(2), _top(2.51), _top(1.0004), _top(1), _top(2.0004)]
PRODUCT_TOP = _top(0.5002)           # every product: |v| <= 0.5001 r + |a b| / 2^270 < 0.5002 r
COLUMN_BOUND = 1 << 63               # a product's column fits the signed 64-bit accumulator
INV256 = pow(FE.R256, -1, R)


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pq") / "pq_reach")
    # -fwrapv: a digit sum that overflowed would wrap on the device, and so must it here
    subprocess.run(["g++", "-O2", "-fwrapv", "-o", exe, os.path.join(ROOT, "tests", "host", "pq_reach_host.cpp")], check=True)

    def run(t, alpha, beta, gamma, ks, lines, has_gate):
        """lines: plain values [w, zinv, z, zrot, l0, gate, f_0.., s_0..].  Returns (report, the results as plain values)"""
        img = lambda v: "%064x" % (v % R * FE.R256 % R)
        head = " ".join(img(v) for v in [alpha, beta, gamma] + [beta * k * 7 for k in ks])
        text = "%d %d %d\n%s\n" % (t, len(lines), 1 if has_gate else 0, head) + "".join(" ".join(img(v) for v in l) + "\n" for l in lines)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == 13 + len(lines)
        return [int(v) for v in out[:13]], [int(v, 16) * INV256 % R for v in out[13:]]

    return run


def _want(t, alpha, beta, gamma, ks, l, has_gate):
    w, zinv, z, zr, l0, gate = l[:6]
    a, b = z, zr
    for j in range(t):
        a = a * ((l[6 + j] + beta * ks[j] * 7 % R * w + gamma) % R) % R
        b = b * ((l[6 + j] + beta * l[6 + t + j] + gamma) % R) % R
    return ((gate if has_gate else 0) + alpha * (a - b) + alpha * alpha % R * (z - 1) % R * l0) % R * zinv % R


@pytest.mark.parametrize("alpha,beta", [(ALPHA, BETA), (0, BETA), (ALPHA, 0), (FE.extremal_multipliers()[0], FE.extremal_multipliers()[2])])
@pytest.mark.parametrize("has_gate", [False, True])
@pytest.mark.parametrize("t", [1, 7])
def test_replay_extremal_images_and_twiddles(replay, t, has_gate, alpha, beta):
    """half values and digit-extremal images in every data position, extremal twiddles and vanishing inverses, t = 1 (one product
    per running product) and t = 7 (seven), alpha = 0 and beta = 0"""
    images = [v * INV256 % R for v in FE.half_values() + FE.digit_extremal() + [1, R - 1, FE.R256, 0]]
    mults = FE.extremal_multipliers() + [1, R - 1]
    rnd = random.Random(1000 * t + has_gate)
    ks = GO.shifts(t)
    lines = []
    for i in range(64):
        l = [mults[i % len(mults)], mults[(i // len(mults) + 3 * i) % len(mults)]]
        l += [images[(5 * i + 3 * c) % len(images)] if i % 4 else rnd.randrange(R) for c in range(4 + 2 * t)]
        lines.append(l)
    rep, got = replay(t, alpha, beta, GAMMA, ks, lines, has_gate)
    assert all(got <= bound for got, bound in zip(rep[:5], RAW_BOUNDS)), (rep[:5], RAW_BOUNDS)
    assert all(got <= bound for got, bound in zip(rep[5:10], TOP_BOUNDS)), (rep[5:10], TOP_BOUNDS)
    assert rep[10] <= NORM and rep[11] <= PRODUCT_TOP and rep[12] < COLUMN_BOUND, rep[10:]
    assert rep[0] and rep[1] and rep[2] and rep[3] and (rep[4] or not (has_gate or alpha)), rep  # every sum was seen
    assert got == [_want(t, alpha, beta, GAMMA, ks, l, has_gate) for l in lines]


# ---- argument errors that need no GPU ------------------------------------------------------------------------------------------
def test_null_context_is_refused_by_every_entry_point():
    lib = K.load_library()
    a = np.zeros((64, 4), dtype=np.uint64)
    p = a.ctypes.data
    assert lib.kzg_coset_extend(None, p, 4, 1, 4, K.KZG_EXTEND_VALUES, 2, p) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_coset_extend_device(None, p, 4, 1, 4, K.KZG_EXTEND_VALUES, 2, p) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_permutation_constraints_coset(None, p, p, p, 2, 2, 1, 4, p, p, p, p, None, p) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_permutation_constraints_coset_device(None, p, p, p, 2, 2, 1, 4, p, p, p, p, None, p) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_vanishing_quotient(None, p, 4, 2, 0, p) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_vanishing_quotient_device(None, p, 4, 2, 0, p) == K.KZG_ERR_INVALID_ARG
    assert lib.kzg_permutation_quotient(None, p, p, p, 2, 1, 2, p, p, p, p, None, 1, p, None) == K.KZG_ERR_INVALID_ARG
    assert (K.KZG_PQ_MAX_COLUMNS, K.KZG_PQ_MAX_LOG_EXT, K.KZG_EXTEND_VALUES, K.KZG_EXTEND_COEFFS) == (7, 3, 0, 1)
    assert C.sizeof(C.c_size_t) == 8
