"""CPU: the host side of the combined openings -- the accumulate step of k_combine_eval as compiled by
g++ against big integers, kzg_combine_claims / kzg_verify_combined on trapdoor-made inputs, their argument errors, and the
export of every new symbol."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import kzg_poly_commit_exploration_amd as K
import open_combined_oracle as CO
import trapdoor_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = K.R_MODULUS
R270 = 1 << 270
NEW_SYMBOLS = ("kzg_open_combined", "kzg_open_combined_submit", "kzg_wait_combined", "kzg_get_combine_ms", "kzg_combine_polys",
               "kzg_evaluate_batch_at", "kzg_combine_claims", "kzg_verify_combined")


# ---------------------------------------------------------------- the accumulate step (fr30_mac), g++ build

@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("r30c") / "libr30c.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "host", "fr30_combine_host.cpp")],
                   check=True)
    return ctypes.CDLL(out)


def _u32x8(v):
    return [(v >> (32 * i)) & 0xffffffff for i in range(8)]


def _run_sum(lib, start, coeffs, mult_values):
    """mult_values: the integers W the digits of the multipliers shall hold (mod r); the harness prepares them as the
    library's host code prepares gamma^i, from the blst_fr image of w = W / 2^270"""
    n = len(coeffs)
    cbuf = (ctypes.c_uint32 * (8 * max(n, 1)))(*[x for c in coeffs for x in _u32x8(c)])
    images = [W * pow(1 << 14, -1, R) % R for W in mult_values]  # w * 2^256 with w * 2^270 = W
    mbuf = (ctypes.c_uint64 * (4 * max(n, 1)))(*[(m >> (64 * i)) & 0xffffffffffffffff for m in images for i in range(4)])
    acc, out, maxima = (ctypes.c_int32 * 9)(), (ctypes.c_uint32 * 8)(), (ctypes.c_int64 * 3)()
    lib.r30c_sum((ctypes.c_uint32 * 8)(*_u32x8(start)), cbuf, mbuf, n, acc, out, maxima)
    value = sum(int(x) << (30 * i) for i, x in enumerate(acc))
    return value, sum(int(w) << (32 * i) for i, w in enumerate(out)), list(maxima)


@pytest.mark.parametrize("count", [1, 2, 3, 255, 256])
def test_accumulate_step_worst_magnitudes(lib, count):
    """sums of `count` products of worst-magnitude operands stay inside the digit bounds stated above fr30_mac, hold the right
    value mod r before the reduction, and leave as its canonical residue"""
    bounds = (ctypes.c_int64 * 3)()
    lib.r30c_bounds(bounds)
    raw_bound, norm_bound, top_bound = list(bounds)
    assert raw_bound == (1 << 30) + 4 < (1 << 31) - (1 << 29)  # what fr30_norm takes
    assert norm_bound == (1 << 29) + 4 and top_bound == 1 << 22
    rng = random.Random(count)
    half = (R - 1) // 2
    for variant in ("all-positive", "all-negative", "random-signs", "edge-multipliers"):
        for start in (0, R - 1):
            coeffs, mults, want = [], [], start
            for k in range(count):
                c = R - 1 if variant != "edge-multipliers" or k % 2 else (1 << 256) - 1  # (a device buffer may hold any 256 bits)
                if variant == "edge-multipliers":  # the ends of what the host's preparation emits: canonical residues
                    W = rng.choice([R - 1, 1, half, half + 1, 0])
                else:  # the multiplier whose product with c is the centred residue of largest magnitude, either sign
                    sign = {"all-positive": 1, "all-negative": -1}.get(variant) or rng.choice([1, -1])
                    target = sign * (half - rng.randrange(4))
                    W = target * R270 * pow(c, -1, R) % R
                coeffs.append(c)
                mults.append(W)
                want += c * W * pow(R270, -1, R)
            value, canonical, maxima = _run_sum(lib, start, coeffs, mults)
            assert (value - want) % R == 0, (variant, start)
            assert canonical == want % R, (variant, start)
            assert maxima[0] <= raw_bound and maxima[1] <= norm_bound and maxima[2] < top_bound, (variant, start, maxima)
            assert abs(value) < 129.1 * R
            if variant in ("all-positive", "all-negative") and count >= 255:
                assert abs(value) > 0.49 * count * R  # the sums really are of worst magnitude


# ---------------------------------------------------------------- the verifier's side, on trapdoor-made inputs

SECRET = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % R


def _point(oracle, v):
    return K.G1Point(oracle.p1_mult(oracle.p1_generator(), v % R))


def _setup(oracle, t, n, seed, gamma=None, polys=None):
    rng = random.Random(seed)
    if polys is None:
        polys = [[rng.randrange(R) for _ in range(n)] for _ in range(t)]
    z = rng.randrange(R)
    gamma = rng.randrange(R) if gamma is None else gamma
    ys = CO.values(polys, z)
    cs = [TO.poly_eval(p, SECRET) for p in polys]
    v = CO.proof_scalar(CO.combine(polys, gamma), z, SECRET)
    proof = _point(oracle, v) if v is not None else K.G1Point(np.zeros(18, dtype=np.uint64))
    return dict(polys=polys, z=K.Scalar(z), gamma=K.Scalar(gamma), ys=[K.Scalar(y) for y in ys], scalars=cs,
                commitments=[_point(oracle, c) for c in cs], proof=proof)


@pytest.fixture(scope="module")
def s_g2():
    return K.srs_g2_at(TO.secret_be(SECRET), 1)


@pytest.mark.parametrize("t", [1, 2, 17])
def test_verify_combined_accepts_and_rejects(oracle, s_g2, t):
    d = _setup(oracle, t, 6, 100 + t)
    c, y = K.combine_claims(d["commitments"], d["ys"], d["gamma"])
    want_c, want_y = CO.combined_claim(d["scalars"], [v.v for v in d["ys"]], d["gamma"].v)
    assert c.compress() == TO.g1_scalar(oracle, want_c) and y.v == want_y
    assert K.verify_proof(c, d["proof"], d["z"], y, s_g2)
    args = (d["commitments"], d["ys"], d["z"], d["gamma"], d["proof"])
    assert K.verify_combined(*args, s_g2)
    for pos in sorted({0, t // 2, t - 1}):
        ys = list(d["ys"])
        ys[pos] = K.Scalar(ys[pos].v + 1)
        assert not K.verify_combined(d["commitments"], ys, d["z"], d["gamma"], d["proof"], s_g2), pos
        cs = list(d["commitments"])
        cs[pos] = _point(oracle, d["scalars"][pos] + 1)
        assert not K.verify_combined(cs, d["ys"], d["z"], d["gamma"], d["proof"], s_g2), pos
    if t > 1:  # (with one polynomial gamma does not enter)
        assert not K.verify_combined(d["commitments"], d["ys"], d["z"], K.Scalar(d["gamma"].v + 1), d["proof"], s_g2)
    else:
        assert K.verify_combined(d["commitments"], d["ys"], d["z"], K.Scalar(d["gamma"].v + 1), d["proof"], s_g2)
    assert not K.verify_combined(d["commitments"], d["ys"], K.Scalar(d["z"].v + 1), d["gamma"], d["proof"], s_g2)
    assert not K.verify_combined(d["commitments"], d["ys"], d["z"], d["gamma"], d["proof"].add(d["commitments"][0]), s_g2)


def test_verify_combined_special_gammas(oracle, s_g2):
    # gamma = 0: only P_0 counts (0^0 = 1)
    d = _setup(oracle, 5, 6, 7, gamma=0)
    c, y = K.combine_claims(d["commitments"], d["ys"], d["gamma"])
    assert c == d["commitments"][0] and y.v == d["ys"][0].v
    assert d["proof"].compress() == TO.proof(oracle, d["polys"][0], d["z"].v, SECRET)
    assert K.verify_combined(d["commitments"], d["ys"], d["z"], d["gamma"], d["proof"], s_g2)
    ys = list(d["ys"])
    ys[3] = K.Scalar(ys[3].v + 1)  # ... so a wrong later value goes unnoticed, a wrong first one does not
    assert K.verify_combined(d["commitments"], ys, d["z"], d["gamma"], d["proof"], s_g2)
    ys[0] = K.Scalar(ys[0].v + 1)
    assert not K.verify_combined(d["commitments"], ys, d["z"], d["gamma"], d["proof"], s_g2)
    # gamma = 1: the plain sums
    d = _setup(oracle, 5, 6, 8, gamma=1)
    c, y = K.combine_claims(d["commitments"], d["ys"], d["gamma"])
    assert c == K.G1Point.sum(d["commitments"]) and y.v == sum(v.v for v in d["ys"]) % R
    assert K.verify_combined(d["commitments"], d["ys"], d["z"], d["gamma"], d["proof"], s_g2)
    # every commitment at infinity (the zero polynomials): the claim is (infinity, 0), the proof infinity
    d = _setup(oracle, 4, 6, 9, polys=[[0] * 6 for _ in range(4)])
    c, y = K.combine_claims(d["commitments"], d["ys"], d["gamma"])
    assert c.is_infinity() and not c.p1.any() and y.v == 0 and d["proof"].is_infinity()
    assert K.verify_combined(d["commitments"], d["ys"], d["z"], d["gamma"], d["proof"], s_g2)
    ys = [K.Scalar(1)] + d["ys"][1:]
    assert not K.verify_combined(d["commitments"], ys, d["z"], d["gamma"], d["proof"], s_g2)


def test_combine_claims_threaded_runs_match_the_plain_sum(oracle):
    """t = 256 is cut into runs joined by Horner in gamma^L: the same claim as the big-integer sum"""
    rng = random.Random(5)
    t = 256
    cs = [rng.randrange(R) for _ in range(t)]
    base = [_point(oracle, c) for c in cs[:8]]  # (eight scalar multiplications by the oracle, reused)
    ys = [K.Scalar(rng.randrange(R)) for _ in range(t)]
    gamma = K.Scalar(rng.randrange(R))
    for count in (255, 256):
        c, y = K.combine_claims([base[i % 8] for i in range(count)], ys[:count], gamma)
        want_c, want_y = CO.combined_claim([cs[i % 8] for i in range(count)], [v.v for v in ys[:count]], gamma.v)
        assert c.compress() == TO.g1_scalar(oracle, want_c) and y.v == want_y


def test_argument_errors_of_the_host_calls(oracle, s_g2):
    lib = K.load_library()
    d = _setup(oracle, 3, 4, 11)
    cs = np.ascontiguousarray(np.stack([c.p1 for c in d["commitments"]]))
    ys = np.ascontiguousarray(np.stack([y.limbs() for y in d["ys"]]))
    z, g, pi = d["z"].limbs(), d["gamma"].limbs(), np.ascontiguousarray(d["proof"].p1)
    g2 = np.ascontiguousarray(s_g2, dtype=np.uint64).reshape(36)
    out_c, out_y, ok = np.zeros(18, dtype=np.uint64), np.zeros(4, dtype=np.uint64), ctypes.c_int(0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.kzg_combine_claims(p(cs), p(ys), 3, p(g), p(out_c), p(out_y)) == K.KZG_OK
    assert lib.kzg_verify_combined(p(cs), p(ys), 3, p(z), p(g), p(pi), p(g2), ctypes.byref(ok)) == K.KZG_OK and ok.value == 1
    big = np.zeros((K.KZG_MAX_COMBINE + 1, 18), dtype=np.uint64)
    big_y = np.zeros((K.KZG_MAX_COMBINE + 1, 4), dtype=np.uint64)
    assert lib.kzg_combine_claims(p(big), p(big_y), K.KZG_MAX_COMBINE, p(g), p(out_c), p(out_y)) == K.KZG_OK
    for t in (0, K.KZG_MAX_COMBINE + 1):
        assert lib.kzg_combine_claims(p(big), p(big_y), t, p(g), p(out_c), p(out_y)) == K.KZG_ERR_INVALID_ARG
        assert lib.kzg_verify_combined(p(big), p(big_y), t, p(z), p(g), p(pi), p(g2), ctypes.byref(ok)) == K.KZG_ERR_INVALID_ARG
    good = [p(cs), p(ys), 3, p(g), p(out_c), p(out_y)]
    for pos in (0, 1, 3, 4, 5):
        args = list(good)
        args[pos] = None
        assert lib.kzg_combine_claims(*args) == K.KZG_ERR_INVALID_ARG, pos
    good = [p(cs), p(ys), 3, p(z), p(g), p(pi), p(g2), ctypes.byref(ok)]
    for pos in (0, 1, 3, 4, 5, 6, 7):
        args = list(good)
        args[pos] = None
        assert lib.kzg_verify_combined(*args) == K.KZG_ERR_INVALID_ARG, pos
    # gamma and the values have to be below r
    not_fr = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    assert lib.kzg_combine_claims(p(cs), p(ys), 3, p(not_fr), p(out_c), p(out_y)) == K.KZG_ERR_INVALID_ARG
    bad_ys = ys.copy()
    bad_ys[2] = not_fr
    assert lib.kzg_combine_claims(p(cs), p(bad_ys), 3, p(g), p(out_c), p(out_y)) == K.KZG_ERR_INVALID_ARG
    # a G2 point off the twist is malformed input, as for kzg_verify_proof
    bad_g2 = g2.copy()
    bad_g2[0] ^= 1
    assert lib.kzg_verify_combined(p(cs), p(ys), 3, p(z), p(g), p(pi), p(bad_g2), ctypes.byref(ok)) == K.KZG_ERR_INVALID_ARG


def test_abi_exports_the_new_symbols():
    lib = K.load_library()
    header = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in K.ABI_SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, header), name
    assert "#define KZG_MAX_COMBINE 256" in header and K.KZG_MAX_COMBINE == 256
    for name in ("open_combined_limbs", "open_combined_submit", "wait_combined", "combine_polys_limbs", "evaluate_batch_at_limbs"):
        assert callable(getattr(K.Engine, name)), name
    assert callable(K.combine_claims) and callable(K.verify_combined)
    # the header says what gamma has to be, and that nothing is hashed here
    section = header[header.index("combined openings"):header.index("#define KZG_MAX_COMBINE")]
    assert "AFTER the commitments and the values" in section and "Nothing is hashed here" in section
