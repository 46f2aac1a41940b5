"""Byte-level restatement of the wire forms the _bytes entry points take, for the tests: records
encoded as 48-byte compressed points and 32-byte big-endian scalars, the sampling specs' bit-reversed order, and each
corruption of an encoding, built deterministically.  Everything here is Python integers over oracle/bigint_twin.py."""
import bigint_twin as T
import cells_oracle as CO
import trapdoor_oracle as TO

P, R = T.P, T.R


# ---- scalars ---------------------------------------------------------------------------------------------------------------
def fr_be(v):
    """a field element as it travels"""
    return (v % R).to_bytes(32, "big")


def fr_be_raw(v):
    """any integer below 2^256 (canonical or not)"""
    return int(v).to_bytes(32, "big")


def fr_list_be(vals):
    return b"".join(fr_be(v) for v in vals)


def limbs_to_be(row):
    """a blst_fr image (4 x u64, Montgomery) -> its 32 big-endian bytes"""
    return fr_be(T.fr_from_mont_limbs([int(x) for x in row]))


def be_to_limbs(b):
    return T.fr_to_mont_limbs(int.from_bytes(b, "big"))


FR_REJECTED = (R, R + 1, (1 << 256) - 1)


# ---- points ----------------------------------------------------------------------------------------------------------------
def p1_to_48(row):
    """a blst_p1 (18 x u64) -> its 48 compressed bytes"""
    return T.g1_compress(T.g1_from_blst_p1_limbs([int(x) for x in row]))


def x_bytes(x, flags):
    """an abscissa below 2^381 under the given flag bits"""
    assert 0 <= x < 1 << 381
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


def largest_curve_x():
    """the largest abscissa below p with a point on the curve (walking down from p - 1)"""
    x = P - 1
    while pow((x * x * x + 4) % P, (P - 1) // 2, P) != 1:
        x -= 1
    return x


def non_residue_x():
    """the least x >= 1 with x^3 + 4 a non-residue"""
    x = 1
    while pow((x * x * x + 4) % P, (P - 1) // 2, P) != P - 1:
        x += 1
    return x


def malformed_points():
    """{class: 48 bytes} -- every way an encoding fails to decode, none left to chance"""
    good = T.g1_compress(T.g1_mul(T.G1, 5))
    small_x = TO._curve_point(1)[0]  # on the curve, so x + p is on the curve mod p and still fits 381 bits
    assert small_x + P < 1 << 381
    return {
        "flag clear": bytes([good[0] & 0x7F]) + good[1:],
        "infinity with x": bytes([0xC0]) + bytes(46) + b"\x01",
        "infinity with sign": bytes([0xE0]) + bytes(47),
        "not on the curve": x_bytes(non_residue_x(), 0x80),
        "x + p": x_bytes(small_x + P, 0x80),
        "x = p": x_bytes(P, 0x80),
    }


def flip_sign(b48):
    """the encoding of -P (P finite)"""
    assert b48[0] & 0x80 and not b48[0] & 0x40
    return bytes([b48[0] ^ 0x20]) + b48[1:]


def plus_torsion(b48, tp):
    """P + tp re-compressed: on the curve, outside G1 when tp is a torsion point"""
    return T.g1_compress(T.g1_add(T.g1_uncompress(b48), tp))


# ---- the bit-reversed order ------------------------------------------------------------------------------------------------
def cells_to_spec(ids, rows, K, t):
    """records (this API's cell id, its l values) -> the sampling specs' view: cell id c with das_cell(K, t, c)[0] = id, the
    values in the order das_cell gives"""
    out_ids, out_rows = [], []
    for j, row in zip(ids, rows):
        c = CO.brp(int(j), K - t)
        ours, order = CO.das_cell(K, t, c)
        assert ours == int(j)
        out_ids.append(c)
        out_rows.append([row[order[i]] for i in range(1 << t)])
    return out_ids, out_rows


def blob_to_spec(vals):
    """a blob's n values in natural order -> the order they travel in: position i holds value brp(i)"""
    n = len(vals)
    k = n.bit_length() - 1
    assert 1 << k == n
    return [vals[CO.brp(i, k)] for i in range(n)]
