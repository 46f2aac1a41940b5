"""CPU: the wire encoders of csrc/wire_enc30.hip.h, compiled for the host with g++, against Python
big integers -- affine records against bigint_twin.g1_compress, blst_fr images against their big-endian bytes -- the round
trips with wire30.hip.h's decoders, and tests/blob_oracle.py against cells_oracle and wire_oracle."""
import ctypes
import os
import random
import subprocess

import pytest

import bigint_twin as T
import blob_oracle as BO
import cells_oracle as CO
import ntt_oracle as NO
import trapdoor_oracle as TO
import wire_oracle as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, R = T.P, T.R
I13 = ctypes.c_int32 * 13
U8 = ctypes.c_uint32 * 8
INFINITY, BAD = 1, 2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("we30") / "libwe30.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "host", "wire_enc30_host.cpp")],
                   check=True)
    L = ctypes.CDLL(out)
    L.we30_g1_encode.restype = None
    L.we30_fr_encode.restype = ctypes.c_uint32
    L.we30_g1_decode.restype = ctypes.c_uint32
    L.we30_fr_decode.restype = ctypes.c_uint32
    return L


def digits(v, lazy=0):
    """v * 2^390 mod p (+ lazy * p) as 13 balanced radix-2^30 digits: the table's record form"""
    n = v * (1 << 390) % P + lazy * P
    out = []
    for _ in range(12):
        d = n & ((1 << 30) - 1)
        if d >= 1 << 29:
            d -= 1 << 30
        out.append(d)
        n = (n - d) >> 30
    out.append(n)
    assert abs(n) < 1 << 29
    return I13(*out)


def encode(lib, pt, lazy=0):
    out = (ctypes.c_uint8 * 48)()
    if pt is T.INF:
        lib.we30_g1_encode(I13(), I13(), out)
    else:
        lib.we30_g1_encode(digits(pt[0], lazy), digits(pt[1], -lazy), out)
    return bytes(out)


def srs_points(count, seed):
    rnd = random.Random(seed)
    s = rnd.randrange(1, R)
    return [T.g1_mul(T.G1, pow(s, rnd.randrange(1 << 20), R)) for _ in range(count)]


def test_points_encode_as_the_oracle_does(lib):
    assert encode(lib, T.INF) == T.g1_compress(T.INF) == bytes([0xC0]) + bytes(47)
    assert encode(lib, T.G1) == T.g1_compress(T.G1)
    for pt in srs_points(200, 11):
        a, b = encode(lib, pt), encode(lib, T.g1_neg(pt))
        assert a == T.g1_compress(pt) and b == T.g1_compress(T.g1_neg(pt))
        assert a[0] & 0x80 and b[0] & 0x80 and not (a[0] | b[0]) & 0x40
        assert (a[0] ^ b[0]) & 0x20 and b == W.flip_sign(a)  # exactly one of the pair carries the sign bit
    # abscissas with leading zero bytes (curve points outside G1: the encoding does not care), and the largest one
    small = [TO._curve_point(x) for x in (0, 1, 2, 255, 256, 1 << 64, 1 << 200, (1 << 373) - 1)]
    x = W.largest_curve_x()
    small.append((x, pow((x ** 3 + 4) % P, (P + 1) // 4, P)))
    for pt in small:
        for q in (pt, T.g1_neg(pt)):
            assert encode(lib, q) == T.g1_compress(q), q
    assert any(T.g1_compress(pt)[1:20] == bytes(19) for pt in small)
    # the record's value may be lazily reduced (negative, or above p): the encoding is that of the residue
    for pt in srs_points(8, 12):
        for lazy in (-1, 1):
            assert encode(lib, pt, lazy) == T.g1_compress(pt)


def fr_encode(lib, v_image):
    limbs = U8(*[(v_image >> (32 * i)) & 0xFFFFFFFF for i in range(8)])
    out = (ctypes.c_uint8 * 32)()
    st = lib.we30_fr_encode(limbs, out)
    return st, bytes(out)


def test_scalars_encode_to_big_endian_bytes(lib):
    rnd = random.Random(13)
    vals = [0, 1, 2, R - 1, R - 2, (1 << 254) - 1, R // 2, R // 2 + 1] + [rnd.randrange(R) for _ in range(2000)]
    for v in vals:
        assert fr_encode(lib, v * T.FR_R % R) == (0, W.fr_be(v)), v
    for image in W.FR_REJECTED + (R + (1 << 200), (1 << 255) + 5):  # an image not below r is not a blst_fr
        st, out = fr_encode(lib, image)
        assert st == BAD and out == W.fr_be(image * pow(T.FR_R, -1, R)), image


def test_round_trips_with_the_decoders(lib):
    rnd = random.Random(14)
    # encode(decode(bytes)) = bytes
    pts = srs_points(40, 15)
    for enc in [T.g1_compress(p) for p in pts] + [W.flip_sign(T.g1_compress(p)) for p in pts[:10]] + [T.g1_compress(T.INF)]:
        x, y = I13(), I13()
        st = lib.we30_g1_decode(enc, x, y)
        assert not st & BAD
        out = (ctypes.c_uint8 * 48)()
        lib.we30_g1_encode(x, y, out)
        assert bytes(out) == enc
    # decode(encode(record)) = the same point
    val = lambda d: sum(int(v) << (30 * i) for i, v in enumerate(d)) * pow(1 << 390, -1, P) % P  # noqa: E731
    for pt in pts[:20]:
        x, y = I13(), I13()
        assert lib.we30_g1_decode(encode(lib, pt), x, y) == 0 and (val(x), val(y)) == pt
    for v in [0, 1, R - 1] + [rnd.randrange(R) for _ in range(500)]:
        image = v * T.FR_R % R
        st, be = fr_encode(lib, image)
        out = U8()
        assert st == 0 and lib.we30_fr_decode(be, out) == 0
        assert sum(int(w) << (32 * i) for i, w in enumerate(out)) == image
        limbs = U8()
        assert lib.we30_fr_decode(W.fr_be(v), limbs) == 0
        out32 = (ctypes.c_uint8 * 32)()
        assert lib.we30_fr_encode(limbs, out32) == 0 and bytes(out32) == W.fr_be(v)


def test_blob_oracle_orders():
    rnd = random.Random(16)
    for n, K_, t in ((16, 5, 2), (64, 7, 0), (8, 3, 3)):
        coeffs = [rnd.randrange(R) for _ in range(n)]
        evals = NO.ntt(coeffs)
        nat = W.fr_list_be(evals)
        spec = W.fr_list_be(W.blob_to_spec(evals))
        assert BO.blob_coefficients(nat, BO.NATURAL) == coeffs == BO.blob_coefficients(spec, BO.BIT_REVERSED)
        M, l = (1 << K_) >> t, 1 << t
        v = CO.cells(coeffs, K_, t)
        assert BO.cells_bytes(coeffs, K_, t, BO.NATURAL) == W.fr_list_be(v)
        sp = BO.cells_bytes(coeffs, K_, t, BO.BIT_REVERSED)
        # the specs' order is the bit-reversed evaluations over the N-domain, cut into cells
        ext = NO.ntt(coeffs + [0] * ((1 << K_) - n))
        assert sp == W.fr_list_be(W.blob_to_spec(ext))
        if 2 * n == 1 << K_:  # ... whose first half is the blob as sent
            assert sp[:32 * n] == spec
        pts = [T.g1_mul(T.G1, j + 1) for j in range(M)]
        got = BO.proofs_bytes(pts, K_, t, BO.BIT_REVERSED)
        for c in range(M):
            assert got[48 * c:48 * c + 48] == T.g1_compress(pts[CO.brp(c, K_ - t)])
        assert BO.proofs_bytes(pts, K_, t, BO.NATURAL) == b"".join(T.g1_compress(p) for p in pts)
