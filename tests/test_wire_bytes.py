"""CPU: the wire decoders of csrc/wire30.hip.h, compiled for the host with g++, against Python big
integers -- compressed G1 points against bigint_twin.g1_uncompress with every rejection class built deterministically,
big-endian scalars against bigint_twin.fr_to_mont_limbs -- and tests/wire_oracle.py against cells_oracle.das_cell and
bigint_twin."""
import ctypes
import os
import random
import subprocess

import pytest

import bigint_twin as T
import cells_oracle as CO
import trapdoor_oracle as TO
import wire_oracle as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, R = T.P, T.R
I13 = ctypes.c_int32 * 13
U8 = ctypes.c_uint32 * 8
INFINITY, BAD = 1, 2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("w30") / "libw30.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "host", "wire30_host.cpp")],
                   check=True)
    L = ctypes.CDLL(out)
    L.w30_g1_decode.restype = ctypes.c_uint32
    L.w30_fr_decode.restype = ctypes.c_uint32
    L.w30_brp.restype = ctypes.c_uint32
    return L


def decode(lib, b48):
    """(status, affine point or None): the digits are x * 2^390 as lazily reduced integers"""
    x, y = I13(), I13()
    st = lib.w30_g1_decode(bytes(b48), x, y)
    val = lambda d: sum(int(v) << (30 * i) for i, v in enumerate(d)) * pow(1 << 390, -1, P) % P  # noqa: E731
    if st & INFINITY:
        assert not any(x) and not any(y)
        return st, T.INF
    assert all(abs(int(v)) <= (1 << 29) + 4 for v in list(x)[:12] + list(y)[:12])  # the table's digit contract
    return st, (val(x), val(y))


def test_points_decode_as_the_oracle_does(lib):
    rnd = random.Random(1)
    pts = [T.g1_mul(T.G1, k) for k in (1, 2, 3, 7, R - 1, R - 2, rnd.randrange(R), rnd.randrange(R))]
    pts += [T.g1_neg(p) for p in pts[:4]]
    pts += list(TO.torsion_points().values()) + list(TO.ORDER3)  # on the curve, outside G1: they decode
    x = W.largest_curve_x()
    assert P - 1 - x == 2
    y = pow((x ** 3 + 4) % P, (P + 1) // 4, P)
    pts += [(x, y), (x, P - y)]
    for pt in pts:
        enc = T.g1_compress(pt)
        assert decode(lib, enc) == (0, T.g1_uncompress(enc)) and T.g1_uncompress(enc) == pt
    assert decode(lib, T.g1_compress(T.INF)) == (INFINITY, T.INF)
    for pt in pts[:6]:  # the sign bit alone decides y
        st, got = decode(lib, W.flip_sign(T.g1_compress(pt)))
        assert st == 0 and got == T.g1_neg(pt)


def test_every_malformed_encoding_is_rejected(lib):
    bad = W.malformed_points()
    assert W.non_residue_x() == 1
    assert set(bad) == {"flag clear", "infinity with x", "infinity with sign", "not on the curve", "x + p", "x = p"}
    for name, enc in bad.items():
        st, _ = decode(lib, enc)
        assert st & BAD, name
    # x + p is congruent to an abscissa of the curve: only the integer comparison rejects it
    xp = int.from_bytes(bytes([bad["x + p"][0] & 0x1F]) + bad["x + p"][1:], "big")
    assert xp >= P and pow(((xp % P) ** 3 + 4) % P, (P - 1) // 2, P) == 1
    # and with the sign bit set, and infinity's flag on a finite x
    assert decode(lib, W.x_bytes(xp, 0xA0))[0] & BAD
    assert decode(lib, W.x_bytes(4, 0xC0))[0] & BAD


def fr_decode(lib, b32):
    out = U8()
    st = lib.w30_fr_decode(bytes(b32), out)
    return st, [int(out[2 * i]) | int(out[2 * i + 1]) << 32 for i in range(4)]


def test_scalars_decode_to_the_blst_fr_image(lib):
    rnd = random.Random(2)
    vals = [0, 1, 2, R - 1, R - 2, 1 << 255 if (1 << 255) < R else R // 2, (1 << 254) - 1] + [rnd.randrange(R) for _ in range(2000)]
    for v in vals:
        assert fr_decode(lib, W.fr_be_raw(v)) == (0, T.fr_to_mont_limbs(v)), v
    for v in W.FR_REJECTED + (R + (1 << 200), (1 << 255) + 5):
        assert v >= R and fr_decode(lib, W.fr_be_raw(v))[0] == BAD, v


def test_bit_reversal(lib):
    for bits in range(0, 14):
        for i in sorted({0, 1, (1 << bits) - 1, (1 << bits) // 3, 5 % (1 << bits)}):
            assert lib.w30_brp(i, bits) == CO.brp(i, bits), (i, bits)
    assert lib.w30_brp(0x12345678, 32) == CO.brp(0x12345678, 32)


def test_wire_oracle_agrees_with_das_cell_and_round_trips():
    rnd = random.Random(3)
    for K_, t in ((13, 6), (8, 0), (6, 6), (5, 2)):
        M, l = (1 << K_) >> t, 1 << t
        ids = [rnd.randrange(M) for _ in range(6)] + [0, M - 1]
        rows = [[rnd.randrange(R) for _ in range(l)] for _ in ids]
        sids, srows = W.cells_to_spec(ids, rows, K_, t)
        for j, row, c, srow in zip(ids, rows, sids, srows):
            ours, order = CO.das_cell(K_, t, c)
            assert ours == j and sorted(order) == list(range(l))
            for i in range(l):  # value i as sent is this API's value brp_t(i), and the other way round
                assert srow[i] == row[CO.brp(i, t)] and row[i] == srow[CO.brp(i, t)]
        assert W.cells_to_spec(*W.cells_to_spec(ids, rows, K_, t), K_, t) == (ids, rows)  # an involution
    blob = [rnd.randrange(R) for _ in range(64)]
    assert W.blob_to_spec(W.blob_to_spec(blob)) == blob and W.blob_to_spec(blob)[1] == blob[32]
    for v in (0, 1, R - 1, rnd.randrange(R)):
        assert W.be_to_limbs(W.fr_be(v)) == T.fr_to_mont_limbs(v) and W.limbs_to_be(T.fr_to_mont_limbs(v)) == W.fr_be(v)
        assert T.fr_from_be_bytes(W.fr_be(v)) == v
    for k in (1, 9, R - 1):
        pt = T.g1_mul(T.G1, k)
        assert W.p1_to_48(T.g1_to_blst_p1_limbs(pt, 7)) == T.g1_compress(pt)
        assert T.g1_uncompress(W.flip_sign(T.g1_compress(pt))) == T.g1_neg(pt)
    assert W.p1_to_48([0] * 18) == T.g1_compress(T.INF)
    tp = TO.torsion_points()[11]
    shifted = T.g1_uncompress(W.plus_torsion(T.g1_compress(T.G1), tp))
    assert T.g1_is_on_curve(shifted) and T.g1_mul(shifted, R) is not T.INF  # r does not kill it: outside G1
    for name, enc in W.malformed_points().items():
        assert len(enc) == 48, name
