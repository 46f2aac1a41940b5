"""CPU: kzg_evaluate_evaluations_batch / kzg_verify_openings_batch / kzg_verify_evaluations_batch
without a device -- the exported symbols and wrapper methods, fr30_inv on the host build of fr30.hip.h against Python's pow,
the oracle's barycentric value against Horner on the interpolated coefficients, and the oracle's two sides under the pairing
of oracle/pairing_twin.py."""
import ctypes
import os
import random
import subprocess

import pytest

import bigint_twin as T
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import pairing_twin as PT
import trapdoor_oracle as TO
import verify_openings_oracle as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = NO.R
B, N = 30, 9
R270 = 1 << 270
I9 = ctypes.c_int32 * 9
S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)
NEW_SYMBOLS = ("kzg_evaluate_evaluations_batch", "kzg_verify_openings_batch", "kzg_verify_openings_lincomb",
               "kzg_verify_evaluations_batch")


def test_library_and_wrapper_have_the_new_entry_points():
    lib = K.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in K.ABI_SYMBOLS
    for name in ("evaluate_evaluations_batch", "verify_openings_batch", "verify_openings_lincomb", "verify_evaluations_batch"):
        assert callable(getattr(K.Engine, name)), name
    header = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    assert "#define KZG_VERIFY_MAX_OPENINGS (1u << 20)" in header


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("r30inv") / "libr30inv.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "host", "fr30_inv_host.cpp")],
                   check=True)
    return ctypes.CDLL(out)


def balanced(v):
    d = []
    for _ in range(N - 1):
        r = v & ((1 << B) - 1)
        if r >= 1 << (B - 1):
            r -= 1 << B
        d.append(r)
        v = (v - r) >> B
    d.append(v)
    return d


def value(d):
    return sum(int(x) << (B * i) for i, x in enumerate(d))


def _check_inverse(lib, digits):
    """digits: a lazy value x * 2^270; fr30_inv returns x^-1 * 2^270, and their product (divided by 2^270) is 2^270"""
    a = value(digits) % R
    x = a * pow(R270, -1, R) % R
    out, prod = I9(), I9()
    lib.r30_inv(I9(*digits), out)
    got = value(list(out))
    assert got % R == pow(x, R - 2, R) * R270 % R, digits
    assert abs(got) <= 0.5001 * R + 1
    assert all(-(1 << 29) <= v < (1 << 29) for v in list(out)[:8])
    lib.r30_mul(I9(*digits), out, prod)
    assert value(list(prod)) % R == (R270 % R if a else 0)  # a * a^-1 = 1 (in the form both carry)


def test_fr30_inv_matches_pow(lib):
    rnd = random.Random(20)
    named = [1, 2, R - 1, (R + 1) // 2, (R - 1) // 2]
    for x in named + [rnd.randrange(1, R) for _ in range(1000)]:
        _check_inverse(lib, balanced(x * R270 % R))
    for x in named:  # the same values as plain integers and as centred (negative) representatives
        _check_inverse(lib, balanced(x))
        _check_inverse(lib, balanced(x - R))
    # digits at the ends of the signed range: what fr30_norm may leave ([-2^29 - 4, 2^29 + 4]) and what a product returns
    lo, hi = -(1 << 29) - 4, (1 << 29) + 4
    for it in range(64):
        d = [rnd.choice([lo, hi, -(1 << 29), (1 << 29) - 1]) for _ in range(8)] + [rnd.randrange(-0x3a00, 0x3a00)]
        if it == 0:
            d = [hi] * 8 + [0x39ff]
        if it == 1:
            d = [lo] * 8 + [-0x39ff]
        if value(d) % R:
            _check_inverse(lib, d)
    out = I9()
    lib.r30_inv(I9(*([0] * 9)), out)
    assert value(list(out)) % R == 0


def test_barycentric_matches_horner_on_the_interpolant():
    rnd = random.Random(21)
    for n in (1, 2, 4, 8, 16, 32, 64):
        evals = [rnd.randrange(R) for _ in range(n)]
        coeffs = NO.intt(evals)
        w = NO.domain_root(NO.log2_exact(n))
        points = [rnd.randrange(R), 0] + [pow(w, j, R) for j in range(n)]
        for z in points:
            assert VO.barycentric(evals, z) == TO.poly_eval(coeffs, z) == NO.barycentric_eval(evals, z), (n, z)
        for j in range(n):
            assert VO.barycentric(evals, pow(w, j, R)) == evals[j]
    # every size up to 64 that is a domain: the sizes above; a non power of two has no domain
    with pytest.raises(AssertionError):
        VO.barycentric([1, 2, 3], 5)


def _records(rnd, polys_n, idx, zs):
    polys = [[rnd.randrange(R) for _ in range(n)] for n in polys_n]
    coms, prfs, ys = VO.trapdoor_records(polys, idx, zs, S)
    return polys, coms, prfs, ys


def test_scalar_sides_hold_and_break():
    rnd = random.Random(22)
    idx = [0, 1, 1, 2, 0, 2, 2]
    z_shared = rnd.randrange(R)
    zs = [z_shared, z_shared, rnd.randrange(R), z_shared, rnd.randrange(R), 0, 1]
    polys, coms, prfs, ys = _records(rnd, [5, 1, 9], idx, zs)
    w = [rnd.randrange(R) for _ in idx]
    assert VO.holds(coms, idx, zs, ys, prfs, w, S)
    y2 = list(ys)
    y2[3] = (y2[3] + 1) % R
    assert not VO.holds(coms, idx, zs, y2, prfs, w, S)
    z2 = list(zs)
    z2[4] = (z2[4] + 1) % R  # (record 2 opens a constant: any point is right for it)
    assert not VO.holds(coms, idx, z2, ys, prfs, w, S)
    p2 = list(prfs)
    p2[0], p2[2] = p2[2], p2[0]
    assert not VO.holds(coms, idx, zs, ys, p2, w, S)
    i2 = list(idx)
    i2[4] = 1
    assert not VO.holds(coms, i2, zs, ys, prfs, w, S)
    # the cancelling pair: y + d and y - d on two records of one commitment at one point pass under EQUAL weights only
    idx3, zs3 = [0, 0], [z_shared, z_shared]
    coms3, prfs3, ys3 = VO.trapdoor_records(polys, idx3, zs3, S)
    bad = [(ys3[0] + 7) % R, (ys3[1] - 7) % R]
    assert VO.holds(coms3, idx3, zs3, bad, prfs3, [5, 5], S)
    assert not VO.holds(coms3, idx3, zs3, bad, prfs3, [5, 6], S)


def test_three_records_under_the_pairing():
    rnd = random.Random(23)
    idx = [0, 1, 0]
    z = rnd.randrange(R)
    zs = [z, z, rnd.randrange(R)]
    polys, coms, prfs, ys = _records(rnd, [4, 3], idx, zs)
    w = [rnd.randrange(R) for _ in idx]
    g1 = lambda v: T.g1_mul(T.G1, v % R)  # noqa: E731
    s_g2 = PT.g2_mul(PT.G2, S)

    def pairing_holds(values):
        lhs, rhs = VO.g1_sides([g1(c) for c in coms], idx, zs, values, [g1(p) for p in prfs], w)
        return PT.pairing_product_is_one([(lhs, s_g2), (T.g1_neg(rhs), PT.G2)])

    assert pairing_holds(ys)
    bad = list(ys)
    bad[1] = (bad[1] + 1) % R
    assert not pairing_holds(bad)
