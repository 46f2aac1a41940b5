"""Case tables for the field and group-law primitives (csrc/field30.hip.h, field30_inv.hip.h, fr30.hip.h, g1_30.hip.h), with
expectations from Python integers only: plain % arithmetic for the fields, oracle/bigint_twin.py for points.  The code
under test never supplies an expectation.  TEST INFRASTRUCTURE ONLY.

tests/test_device_prims.py runs every table through the g++ build of the headers (tests/host/*.cpp),
tests/test_device_prims_gpu.py through the device build (tests/device/prims.hip); both assert what `check` says here.

Conventions
  * Operands are built as integers and cut into balanced digits (test_field30.balanced / test_fr30.balanced).
  * A representative of x with magnitude up to m: x * 2^390 mod p + k p with |value| < m p.  "extreme" takes the smallest or
    the largest such k, "random" any.  Half of every group-law table is extreme, half random.
  * Group-law operands: points [k]G for small k; XYZZ operands with a random z, X up to 2.6 p, Y up to 1.3 p, ZZ and ZZZ up
    to 0.7 p (the magnitudes stated at the top of g1_30.hip.h); affine operands of xyzz30_madd with x up to 2 p and y up to
    1.3 p (what pair_sum leaves); operands of pair_classify / pair_sum below 0.62 p (table points: srs_io.hip reduces
    them with one product).
  * fq_sqr and fq_mul_sub take weakly normalised digits only (|digit| <= 2^29 + 4: the doubled operand of the square and
    the column bound of the double product, field30.hip.h), so where fq_mul gets the raw sum or difference of two values,
    these two get its fq_norm -- R (Q - X3) - Y1 PPP is fed exactly that by the group law.
  * Quad tables hold whole waves: 16 consecutive cases are the 16 quads of one wave, and `where` names the composition and
    the quad's position.  Results come back once per lane (4 x 52 ints per case).
"""
import random

import numpy as np

import bigint_twin as T
from test_field30 import balanced, value
from test_fr30 import balanced as balanced9

P = T.P
R = T.R
RQ = 1 << 390
RQ_INV = pow(RQ, -1, P)
R270 = 1 << 270
B = 30
BIG = (1 << 29) + 4  # weakly normalised digit
HALF = 1 << 29
KINDS = ("general", "equal", "opposite", "b_inf", "acc_inf", "both_inf")
LIVE = ("general", "equal", "opposite")
PAIR_NAMES = {0: "None", 1: "Add", 2: "Double", 3: "Cancel", 4: "OnlyA", 5: "OnlyB"}


class Table:
    """rows: one list of ints per case (the input record); wants: what `check(row, want, out)` compares the output record
    with (it returns None, or a message); kinds / where: names for a failure report; host: how the g++ build produces the
    same output records (None: the export of the same name)."""

    def __init__(self, name, op, ow, check, host=None, batches=None):
        self.name, self.op, self.ow, self.check, self.host, self.batches = name, op, ow, check, host, batches
        self.rows, self.wants, self.kinds, self.where = [], [], [], []

    def add(self, kind, row, want, where=""):
        self.rows.append(row)
        self.wants.append(want)
        self.kinds.append(kind)
        self.where.append(where)

    @property
    def n(self):
        return len(self.rows)

    @property
    def iw(self):
        return len(self.rows[0])

    def inputs(self):
        assert self.n <= 4096 and all(len(r) == self.iw for r in self.rows), self.name
        a = np.array(self.rows, dtype=np.int64)
        assert a.min() >= -(1 << 31) and a.max() < (1 << 32), self.name
        return np.ascontiguousarray(a.astype(np.uint32).view(np.int32))  # unsigned words travel as their int32 image


def failures(table, out):
    """[(case index, message)] for the output records `out` (n x ow)"""
    bad = []
    for i in range(table.n):
        msg = table.check(table.rows[i], table.wants[i], [int(v) for v in out[i]])
        if msg:
            bad.append((i, msg))
    return bad


# ---- integers ------------------------------------------------------------------------------------------------------------
def norm_py(d):
    """the parallel carry pass of fq_norm / fr30_norm on Python integers (no 32-bit wrap-around)"""
    n = len(d)
    c = [(x + HALF) >> B for x in d[:n - 1]]
    return [d[0] - (c[0] << B)] + [d[i] - (c[i] << B) + c[i - 1] for i in range(1, n - 1)] + [d[n - 1] + c[n - 2]]


def rep_range(v0, m10, mod):
    """the smallest and the largest k with |v0 + k mod| < m10 / 10 mod"""
    bound = m10 * mod // 10
    lo = (-bound - v0) // mod + 1
    hi = -((v0 - bound) // mod) - 1
    assert abs(v0 + lo * mod) < bound and abs(v0 + hi * mod) < bound and lo <= hi
    assert abs(v0 + (lo - 1) * mod) >= bound and abs(v0 + (hi + 1) * mod) >= bound
    return lo, hi


def rep(x, m10, rng, extreme):
    """digits of a representative of x (Montgomery 2^390) of magnitude below m10 / 10 p"""
    v0 = x * RQ % P
    lo, hi = rep_range(v0, m10, P)
    k = rng.choice((lo, hi)) if extreme else rng.randrange(lo, hi + 1)
    return balanced(v0 + k * P)


def mont_py(a, b):
    """the exact integer fq_mul returns for the integers a, b: (a b + m p) / 2^390 with m the balanced-digit residue"""
    return mont_t(a * b)


def mont_t(t):
    """(t + m p) / 2^390 for the column sums t of one Montgomery reduction (fq_mul: a b; fq_mul_sub: a b - c d)"""
    u = (-t * pow(P, -1, RQ)) % RQ
    m = 0
    for i in range(13):
        r = u & ((1 << B) - 1)
        if r >= HALF:
            r -= 1 << B
        m += r << (B * i)
        u = (u - r) >> B
    assert (t + m * P) % RQ == 0
    return (t + m * P) >> 390


def limbs(v, n):
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def unlimbs(w):
    return sum((int(x) & 0xffffffff) << (32 * i) for i, x in enumerate(w))


def digits_ok(d, lo=-HALF, hi=HALF - 1, upto=12):
    return all(lo <= x <= hi for x in d[:upto])


# ---- Fp tables ---------------------------------------------------------------------------------------------------------------
def _lazy(rng, bits=383):
    return rng.randrange(-(1 << bits), 1 << bits)


def _check_product(exact):
    """out = exact(row) / 2^390 (mod p); digits 0..11 in [-2^29, 2^29); |out| < 0.62 p + |exact| / 2^390"""
    def check(row, want, out):
        t = exact(row)
        v = value(out)
        if (v * RQ - t) % P:
            return "value: got %d" % v
        if not digits_ok(out):
            return "digits outside [-2^29, 2^29): %s" % out
        if not abs(v) < 62 * P // 100 + (abs(t) >> 390) + 1:
            return "magnitude %.3f p" % (v / P)
    return check


def _weak(d):
    out = norm_py(d)
    assert value(out) == value(d) and digits_ok(out, -BIG, BIG)
    return out


def _field_operand_sets(rng, weak_only):
    """(kind, operand digit lists): the operands one product case is drawn from"""
    pd = balanced(P)
    sets = []
    for sa in (1, -1):
        for sb in (1, -1):
            a = [sa * BIG] * 12 + [1 << 24] if weak_only else [sa * 2 * BIG] * 12 + [1 << 27]
            sets.append(("adversarial", a, [sb * BIG] * 12 + [1 << 27 if not weak_only else 1 << 24]))
    a = [(BIG if x >= 0 else -BIG) * (1 if weak_only else 2) for x in pd[:12]] + [0]
    sets.append(("adversarial", a, [BIG] * 12 + [0]))
    sets.append(("adversarial", a, [(BIG if x >= 0 else -BIG) for x in pd[:12]] + [0]))
    for it in range(64):
        x, y, z = (balanced(_lazy(rng, 381)) for _ in range(3))
        raw = [p - q if it & 1 else p + q for p, q in zip(x, y)]
        if weak_only:
            raw = _weak(raw)
        sets.append(("raw_sum", raw, z) if it & 2 else ("raw_sum", z, raw))
    for sa in (1, -1):
        for sb in (1, -1):
            for _ in range(4):
                sets.append(("mag_2^385", balanced(sa * ((1 << 385) - rng.randrange(1 << 380))),
                             balanced(sb * ((1 << 385) - rng.randrange(1 << 380)))))
    small = [0, 1, -1, P, -P]
    for a in small:
        for b in small + [_lazy(rng)]:
            sets.append(("small", balanced(a), balanced(b)))
    for _ in range(512):
        sets.append(("random", balanced(_lazy(rng)), balanced(_lazy(rng))))
    return sets


def t_fq_mul():
    t = Table("fq_mul", "fq_mul", 13, _check_product(lambda r: value(r[:13]) * value(r[13:26])))
    for kind, a, b in _field_operand_sets(random.Random(1001), False):
        t.add(kind, a + b, None)
    return t


def t_fq_sqr():
    t = Table("fq_sqr", "fq_sqr", 13, _check_product(lambda r: value(r) ** 2))
    for kind, a, b in _field_operand_sets(random.Random(1002), True):
        t.add(kind, a, None)
        if kind != "random":
            t.add(kind, b, None)
    return t


def t_fq_mul_sub():
    t = Table("fq_mul_sub", "fq_mul_sub", 13,
              _check_product(lambda r: value(r[:13]) * value(r[13:26]) - value(r[26:39]) * value(r[39:52])))
    rng = random.Random(1003)
    sets = _field_operand_sets(rng, True)
    for i, (kind, a, b) in enumerate(sets):
        _, c, d = sets[(i * 7 + 3) % len(sets)] if kind != "adversarial" else (None, [-x for x in a[:12]] + [a[12]], b)
        t.add(kind, a + b + c + d, None)
    return t


def _check_same_value(bound):
    def check(row, want, out):
        d = row[:len(out)]
        if value(out) != value(d):
            return "value changed: %d -> %d" % (value(d), value(out))
        if not digits_ok(out, -bound, bound, len(out) - 1):
            return "digits above 2^29 + 4: %s" % out
        if want is not None and out != want:
            return "digits %s, expected %s" % (out, want)
    return check


def _digit_rows(rng, n, span, top, count):
    rows = [[s * (span - 1)] * (n - 1) + [s * top] for s in (1, -1)]
    rows.append([(span - 1) * (1 if i & 1 else -1) for i in range(n - 1)] + [0])
    rows.append([HALF] * (n - 1) + [0])          # every digit carries
    rows.append([-HALF - 1] * (n - 1) + [0])
    rows.append([HALF - 1] * (n - 1) + [0])      # none does
    rows.append([0] * n)
    for _ in range(count):
        rows.append([rng.randrange(-span + 1, span) for _ in range(n - 1)] + [rng.randrange(-top, top + 1)])
    return rows


def t_fq_norm():
    t = Table("fq_norm", "fq_norm", 13, _check_same_value(BIG))
    for row in _digit_rows(random.Random(1004), 13, 3 << 29, 1 << 26, 500):
        t.add("digits<3*2^29", row, norm_py(row))
    return t


def t_fq_norm_wide():
    """digits over the whole int32 range (X3 = RR - PPP - 2 Q: sums of four); where fq_norm applies, the same digits"""
    t = Table("fq_norm_wide", "fq_norm_wide", 13, _check_same_value(BIG))
    rng = random.Random(1005)
    for row in _digit_rows(rng, 13, 3 << 29, 1 << 26, 200):
        t.add("digits<3*2^29", row, norm_py(row))
    rows = _digit_rows(rng, 13, 1 << 31, 1 << 26, 500)
    rows.append([-(1 << 31)] * 12 + [5])
    rows.append([(1 << 31) - 1] * 12 + [-5])
    for row in rows:
        t.add("digits<=2^31", row, None)
    return t


def t_fq_neg():
    def check(row, want, out):
        if out != want:
            return "digits %s, expected %s" % (out, want)
    t = Table("fq_neg_cneg", "fq_cneg", 13, check)
    rng = random.Random(1006)
    for row in _digit_rows(rng, 13, 1 << 31, 1 << 30, 200):
        for neg in (0, 1):
            t.add("cneg%d" % neg, row + [neg], [-x for x in row] if neg else row)
    return t


def t_fq_neg_plain():
    def check(row, want, out):
        if out != want:
            return "digits %s, expected %s" % (out, want)
    t = Table("fq_neg", "fq_neg", 13, check)
    for row in _digit_rows(random.Random(1007), 13, 1 << 31, 1 << 30, 200):
        t.add("neg", row, [-x for x in row])
    return t


def t_fq_canon_digits():
    def check(row, want, out):
        if out != want:
            return "digits %s, expected %s" % (out, want)
    t = Table("fq_canon_digits", "fq_canon_digits", 13, check)
    rng = random.Random(1008)
    rows = _digit_rows(rng, 13, BIG + 1, 1 << 26, 200) + _digit_rows(rng, 13, 2 * BIG + 1, 1 << 26, 200)
    rows += [balanced(k * P) for k in range(-3, 4)]
    for row in rows:
        t.add("digits", row, balanced(value(row)))
    return t


def t_fq_is_zero():
    def check(row, want, out):
        if out[0] != want:
            return "is_zero = %d for %+.4f p (%s a multiple of p)" % (out[0], value(row) / P, "" if want else "not")
    t = Table("fq_is_zero", "fq_is_zero", 1, check)
    rng = random.Random(1009)
    for k in range(-3, 4):
        d = balanced(k * P)
        t.add("%dp canonical" % k, d, 1)
        for _ in range(8):
            u = _lazy(rng, 382)
            raw = [x - y for x, y in zip(balanced(u), balanced(u - k * P))]
            nd = _weak(raw)
            assert value(nd) == k * P
            t.add("%dp norm(raw difference)" % k, nd, 1)
        for j, up in ((11, 1), (11, -1), (10, 1), (3, 1), (7, -1)):
            e = list(d)
            e[j] += up << B
            e[j + 1] -= up
            t.add("%dp re-split at digit %d" % (k, j), e, 1)
        # near misses: the same digit 0 as k p, another integer below 3.5 p
        made = 0
        while made < 24:
            j = rng.randrange(1, 13)
            v = k * P + rng.choice((-1, 1)) * (rng.randrange(1, 1 << 29) if made & 1 else 1) * (1 << (B * j))
            if v % P == 0 or abs(v) >= 35 * P // 10:
                continue
            nd = balanced(v)
            assert nd[0] == d[0]
            t.add("near miss of %dp" % k, nd, 0)
            made += 1
    for _ in range(512):
        v = rng.randrange(-35 * P // 10 + 1, 35 * P // 10)
        t.add("random", balanced(v), 1 if v % P == 0 else 0)
    return t


def t_fq_from_u32x12():
    def check(row, want, out):
        if value(out) != want:
            return "value %d, expected 64 s = %d" % (value(out), want)
        if not digits_ok(out, -HALF, HALF):
            return "digits above 2^29: %s" % out
    t = Table("fq_from_u32x12", "fq_from_u32x12", 13, check)
    rng = random.Random(1010)
    for s in [0, 1, P - 1, P, 2 * P - 1] + [rng.randrange(2 * P) for _ in range(300)]:
        t.add("s", limbs(s, 12), 64 * s)
    return t


def t_fq_to_u32x12():
    def check(row, want, out):
        if unlimbs(out) != want:
            return "words %x, expected %x" % (unlimbs(out), want)
    t = Table("fq_to_u32x12", "fq_to_u32x12", 12, check)
    rng = random.Random(1011)
    i64 = pow(64, -1, P)
    for it, s in enumerate([0, 1, P - 1, P, 2 * P - 1] + [rng.randrange(2 * P) for _ in range(300)]):
        t.add("64 s", balanced(64 * s), s % P)
        v = 64 * s + (it % 7 - 3) * P  # lazy spellings, negative ones included
        t.add("64 s + k p", balanced(v), v * i64 % P)
    return t


def t_fq_canon_half():
    """fq_canonical_integer, then fq_digits_greater against fq_const_half(): the sign bit of the wire format"""
    def check(row, want, out):
        if out[:13] != balanced(want):
            return "canonical integer %s, expected %s" % (out[:13], balanced(want))
        if out[13] != (1 if want > (P - 1) // 2 else 0):
            return "greater-than-half flag %d for y = %d" % (out[13], want)
    t = Table("fq_canonical_integer+fq_digits_greater", "fq_canon_half", 14, check)
    rng = random.Random(1012)
    for y in [0, (P - 1) // 2, (P + 1) // 2, P - 1, 1, (P - 1) // 2 - 1, (P + 1) // 2 + 1] + [rng.randrange(P) for _ in range(100)]:
        v0 = y * RQ % P
        for k in range(-4, 3):
            t.add("y + %dp" % k, balanced(v0 + k * P), y)
    return t


def t_fq_inv():
    def check(row, want, out):
        v = value(out)
        if (v - want * RQ) % P:
            return "value: got %d" % v
        if not digits_ok(out):
            return "digits outside [-2^29, 2^29): %s" % out
        if not abs(v) < 63 * P // 100:
            return "magnitude %.3f p" % (v / P)
    t = Table("fq_inv", "fq_inv", 13, check)
    rng = random.Random(1013)
    for it, x in enumerate([0, 1, P - 1, 2] * 4 + [rng.randrange(1, P) for _ in range(64)]):
        v = x * RQ % P + ((it * 3) % 7 - 4) * P
        t.add("x=%s" % (x if x < 3 else ("-1" if x == P - 1 else "random")), balanced(v), pow(x, -1, P) if x else 0)
    t.add("x=0", [0] * 13, 0)
    return t


# ---- Fr tables ---------------------------------------------------------------------------------------------------------------
def value9(d):
    return sum(int(x) << (B * i) for i, x in enumerate(d))


def t_fr30_mul():
    def check(row, want, out):
        a, b, v = value9(row[:9]), value9(row[9:]), value9(out)
        if (v * R270 - a * b) % R:
            return "value: got %d" % v
        if not digits_ok(out, upto=8):
            return "digits outside [-2^29, 2^29): %s" % out
        if not abs(v) <= 5001 * R // 10000 + (abs(a * b) >> 270) + 1:
            return "magnitude %.4f r" % (v / R)
    t = Table("fr30_mul", "fr30_mul", 9, check)
    rng = random.Random(1101)
    for sa in (1, -1):
        for sb in (1, -1):
            for ba, bb in ((264, 264), (268, 260), (258, 269), (255, 255)):  # |a| |b| < 2^528
                for _ in range(8):
                    a = sa * ((1 << ba) - 1 - rng.randrange(1 << (ba - 4)))
                    b = sb * ((1 << bb) - 1 - rng.randrange(1 << (bb - 4)))
                    t.add("magnitude 2^%d x 2^%d" % (ba, bb), balanced9(a) + balanced9(b), None)
            t.add("extreme digits", [sa * (1 << 30)] * 8 + [1 << 20] + [sb * BIG] * 8 + [1 << 20], None)
    for it in range(200):
        a1, a2, b = (balanced9(rng.randrange(-(1 << 258), 1 << 258)) for _ in range(3))
        a = [x + y for x, y in zip(a1, a2)]
        if it % 4 == 0:
            a = [rng.choice([-(1 << 30), 1 << 30]) for _ in range(8)] + [a[8]]
            b = [rng.choice([-BIG, BIG]) for _ in range(8)] + [b[8]]
        t.add("raw_sum", a + b if it & 1 else b + a, None)
    for a in (0, 1, -1, R, -R):
        for b in (0, 1, -1, R, rng.randrange(R)):
            t.add("small", balanced9(a) + balanced9(b), None)
    for _ in range(400):
        bits = rng.choice([200, 255, 258, 262])
        t.add("random", balanced9(rng.randrange(-(1 << bits), 1 << bits)) + balanced9(rng.randrange(-(1 << bits), 1 << bits)), None)
    return t


def t_fr30_norm():
    t = Table("fr30_norm", "fr30_norm", 9, _check_same_value(BIG))
    for row in _digit_rows(random.Random(1102), 9, 3 << 29, 1 << 26, 400):
        t.add("digits<3*2^29", row, norm_py(row))
    return t


def t_fr30_from_limbs():
    def check(row, want, out):
        if value9(out) != want:
            return "value %d, expected %d" % (value9(out), want)
        if not digits_ok(out, -BIG, BIG, 8):
            return "digits above 2^29 + 4: %s" % out
    t = Table("fr30_from_limbs", "fr30_from_limbs", 9, check)
    rng = random.Random(1103)
    edge = [0, 1, R - 1, R, R + 1, (1 << 256) - 1, 1 << 255, (1 << 255) - 1, R // 2, 2 * R - 1, 2 * R]
    for v in edge + [rng.randrange(1 << 256) for _ in range(400)] + [rng.randrange(1 << rng.randrange(1, 256)) for _ in range(100)]:
        t.add("integer", limbs(v, 8), v)
    return t


def _splits9(d, rng):
    """the same integer in other digits: a unit moved between neighbours, and the weakly normalised extremes"""
    out = [list(d)]
    for j, up in ((0, 1), (3, -1), (7, 1), (7, -1), (rng.randrange(8), rng.choice((1, -1)))):
        e = list(d)
        e[j] += up << B
        e[j + 1] -= up
        out.append(e)
    e = list(d)
    for j in range(8):  # every digit pushed to the far side of its weak range where it can go
        if e[j] < -HALF + 4:
            e[j] += 1 << B
            e[j + 1] -= 1
    out.append(e)
    assert all(value9(x) == value9(d) for x in out)
    return out


def t_fr30_to_limbs():
    def check(row, want, out):
        if unlimbs(out) != want:
            return "words %x, expected %x (v = %+.6f r)" % (unlimbs(out), want, value9(row) / R)
    t = Table("fr30_to_limbs", "fr30_to_limbs", 8, check)
    rng = random.Random(1104)
    for v in [-R + 1, -1, 0, 1, R - 1, R, R + 1, 2 * R - 1, -(R // 2), R + R // 2]:
        for e in _splits9(balanced9(v), rng):
            t.add("edge %+.3f r" % (v / R), e, v % R)
    for it in range(600):
        prod = rng.randrange(-5001 * R // 10000, 5001 * R // 10000 + 1)  # what fr30_mul leaves
        v = prod + (rng.randrange(R) if it & 1 else 0)                    # ... plus at most one canonical coefficient
        d = balanced9(v)
        t.add("product", d if it % 3 else _splits9(d, rng)[-2], v % R)
    return t


def t_fr30_abs_to_limbs():
    def check(row, want, out):
        v = value9(row)
        if unlimbs(out[:8]) != abs(v) or out[8] != (1 if v < 0 else 0):
            return "|v| = %x sign %d, expected %x sign %d" % (unlimbs(out[:8]), out[8], abs(v), v < 0)
    t = Table("fr30_abs_to_limbs", "fr30_abs_to_limbs", 9, check)
    rng = random.Random(1105)
    for v in [0, 1, -1, (R - 1) // 2, -(R - 1) // 2]:
        for e in _splits9(balanced9(v), rng):
            t.add("edge", e, None)
    for it in range(600):
        v = rng.randrange(-(R // 2) - (R >> 31), R // 2 + (R >> 31) + 1)
        t.add("product", balanced9(v), None)
    return t


def t_fr30_inv():
    def check(row, want, out):
        v = value9(out)
        if (v - want * R270) % R:
            return "value: got %d" % v
        if not any(row) and any(out):
            return "inverse of the digits 0 is %s, not the digits 0" % out
        if not digits_ok(out, upto=8):
            return "digits outside [-2^29, 2^29): %s" % out
        if not abs(v) <= 5002 * R // 10000:
            return "magnitude %.4f r" % (v / R)
    t = Table("fr30_inv", "fr30_inv", 9, check)
    rng = random.Random(1106)
    for it, x in enumerate([0, 0, 1, R - 1, 1, R - 1] + [rng.randrange(1, R) for _ in range(64)]):
        v = x * R270 % R
        v -= R if (it & 1 and it > 0) else 0  # both signs
        t.add("x=%s" % (x if x < 2 else ("-1" if x == R - 1 else "random")), balanced9(v), pow(x, -1, R) if x else 0)
    return t


# ---- points --------------------------------------------------------------------------------------------------------------------
_MULTIPLES = [None]


def kG(k):
    """[k]G for small k of either sign"""
    while len(_MULTIPLES) <= abs(k):
        _MULTIPLES.append(T.g1_add(_MULTIPLES[-1], T.G1))
    pt = _MULTIPLES[abs(k)]
    return T.g1_neg(pt) if k < 0 else pt


def xyzz_digits(pt, rng, extreme):
    """52 ints: X, Y, ZZ, ZZZ of pt with a random z and lazy representatives; exact zeros for infinity"""
    if pt is None:
        return [0] * 52
    z = rng.randrange(1, P)
    zz, zzz = z * z % P, z * z * z % P
    return (rep(pt[0] * zz % P, 26, rng, extreme) + rep(pt[1] * zzz % P, 13, rng, extreme) + rep(zz, 7, rng, extreme) +
            rep(zzz, 7, rng, extreme))


def affine_digits(pt, rng, extreme, mx=20, my=13):
    if pt is None:
        return [0] * 26
    return rep(pt[0], mx, rng, extreme) + rep(pt[1], my, rng, extreme)


def xyzz_point(d):
    """the affine point behind 52 digits (None for ZZ == 0 as an integer), without any check"""
    X, Y, ZZ, ZZZ = (value(d[13 * i:13 * i + 13]) for i in range(4))
    if ZZ % P == 0 or ZZZ % P == 0:
        return None
    return X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P


def check_xyzz(out, want):
    """the output contract of the group law for one 52-int result"""
    if want is None:
        return None if not any(out) else "expected infinity as exact zeros, got %s" % out
    X, Y, ZZ, ZZZ = (value(out[13 * i:13 * i + 13]) for i in range(4))
    if ZZ % P == 0 or ZZZ % P == 0:
        return "ZZ or ZZZ is zero mod p for a finite sum"
    got = (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P)
    if got != want:
        return "point (%x.., %x..), expected (%x.., %x..)" % (got[0] >> 320, got[1] >> 320, want[0] >> 320, want[1] >> 320)
    if pow(ZZ * RQ_INV, 3, P) != pow(ZZZ * RQ_INV, 2, P):
        return "ZZ^3 != ZZZ^2"
    for i in range(4):
        if not digits_ok(out[13 * i:13 * i + 13], -BIG, BIG):
            return "digits above 2^29 + 4 in coordinate %d: %s" % (i, out[13 * i:13 * i + 13])
    for name, v, m10 in (("X", X, 26), ("Y", Y, 13), ("ZZ", ZZ, 7), ("ZZZ", ZZZ, 7)):
        if not abs(v) < m10 * P // 10:
            return "|%s| = %.3f p, stated bound %.1f p" % (name, abs(v) / P, m10 / 10)


def operand_pair(kind, rng):
    """(acc point, b point) of one case kind: multiples of G; the sum of a general pair is never exceptional"""
    k = rng.randrange(1, 40)
    j = rng.choice([x for x in range(-40, 41) if x not in (0, k, -k)])
    return {"general": (kG(k), kG(j)), "equal": (kG(k), kG(k)), "opposite": (kG(k), kG(-k)), "b_inf": (kG(k), None),
            "acc_inf": (None, kG(j)), "both_inf": (None, None)}[kind]


def _check_point(row, want, out):
    return check_xyzz(out, want)


def t_madd():
    t = Table("xyzz30_madd", "madd", 52, _check_point)
    rng = random.Random(1201)
    for it in range(768):
        kind, neg, extreme = KINDS[it % 6], (it // 6) & 1, bool((it // 12) & 1)
        a, b = operand_pair(kind, rng)
        # the point handed over is negated by the call when neg: hand over -b then
        row = xyzz_digits(a, rng, extreme) + affine_digits(T.g1_neg(b) if neg else b, rng, extreme) + [neg]
        t.add("%s neg=%d %s" % (kind, neg, "extreme" if extreme else "random"), row, T.g1_add(a, b))
    return t


def _add_rows(seed, n):
    rng = random.Random(seed)
    for it in range(n):
        kind, extreme = KINDS[it % 6], bool((it // 6) & 1)
        a, b = operand_pair(kind, rng)
        yield "%s %s" % (kind, "extreme" if extreme else "random"), xyzz_digits(a, rng, extreme) + xyzz_digits(b, rng, extreme), T.g1_add(a, b)


def t_add():
    t = Table("xyzz30_add", "add", 52, _check_point)
    for kind, row, want in _add_rows(1202, 768):
        t.add(kind, row, want)
    return t


def t_add_call():
    t = Table("xyzz30_add_call", "add_call", 52, _check_point)
    for kind, row, want in _add_rows(1203, 384):
        t.add(kind, row, want)
    return t


def t_dbl():
    t = Table("xyzz30_dbl_inplace", "dbl", 52, _check_point)
    rng = random.Random(1204)
    for it in range(256):
        extreme = bool(it & 1)
        if it % 8 == 0:
            t.add("infinity", [0] * 52, None)
        elif it % 8 == 1:  # Y a multiple of p (no such point in the group; the formulas must still answer infinity)
            d = xyzz_digits(kG(rng.randrange(1, 40)), rng, extreme)
            d[13:26] = balanced(rng.choice((-1, 0, 1)) * P)
            t.add("Y = k p", d, None)
        else:
            pt = kG(rng.randrange(1, 40))
            t.add("finite %s" % ("extreme" if extreme else "random"), xyzz_digits(pt, rng, extreme), T.g1_add(pt, pt))
    return t


# ---- chains: outputs feed inputs ---------------------------------------------------------------------------------------------
def chain_points(rng):
    """16 operands: P, P (doubling), -2P (back to infinity), infinity, then general points with two more infinities"""
    k = rng.randrange(1, 20)
    seq = [kG(k), kG(k), kG(-2 * k), None, kG(rng.randrange(1, 20)), None]
    seq += [kG(rng.choice((-1, 1)) * rng.randrange(1, 20)) for _ in range(9)] + [None]
    partial, acc = [], None
    for pt in seq:
        acc = T.g1_add(acc, pt)
        partial.append(acc)
    return seq, partial


def _check_chain(lanes):
    def check(row, want, out):
        for s in range(16):
            rec = out[s * lanes * 52:(s + 1) * lanes * 52]
            for q in range(1, lanes):
                if rec[q * 52:(q + 1) * 52] != rec[:52]:
                    return "step %d: lane %d of the quad differs from lane 0" % (s, q)
            msg = check_xyzz(rec[:52], want[s])
            if msg:
                return "step %d: %s" % (s, msg)
    return check


def t_chain_madd():
    t = Table("chain xyzz30_madd", "chain_madd", 16 * 52, _check_chain(1))
    rng = random.Random(1205)
    for it in range(64):
        seq, partial = chain_points(rng)
        extreme = bool(it & 1)
        row = []
        for pt in seq:
            neg = rng.randrange(2)
            row += affine_digits(T.g1_neg(pt) if neg else pt, rng, extreme) + [neg]
        t.add("chain %s" % ("extreme" if extreme else "random"), row, partial)
    return t


def _chain_xyzz_rows(seed, n):
    rng = random.Random(seed)
    for it in range(n):
        seq, partial = chain_points(rng)
        extreme = bool(it & 1)
        yield "chain %s" % ("extreme" if extreme else "random"), [v for pt in seq for v in xyzz_digits(pt, rng, extreme)], partial


def _host_chain_quad(run, table):
    out = run("chain_add", table.inputs(), 16 * 52)
    return np.repeat(out.reshape(table.n, 16, 1, 52), 4, axis=2).reshape(table.n, 16 * 4 * 52)


def t_chain_add():
    t = Table("chain xyzz30_add", "chain_add", 16 * 52, _check_chain(1))
    for kind, row, want in _chain_xyzz_rows(1206, 64):
        t.add(kind, row, want)
    return t


def t_chain_quad(dense):
    t = Table("chain xyzz30_add_quad" + ("_dense" if dense else ""), "chain_quad" + ("_dense" if dense else ""), 16 * 4 * 52,
              _check_chain(4), host=_host_chain_quad)
    for i, (kind, row, want) in enumerate(_chain_xyzz_rows(1207 + dense, 64)):
        t.add(kind, row, want, "wave %d quad %d" % (i // 16, i % 16))
    return t


# ---- affine pairs ----------------------------------------------------------------------------------------------------------------
def _pair_case(kind, rng, extreme):
    """(a point as handed over, nega, b point as handed over, negb) for an operand kind, signs drawn at random"""
    a, b = operand_pair(kind, rng)
    nega, negb = rng.randrange(2), rng.randrange(2)
    return (T.g1_neg(a) if nega else a), nega, (T.g1_neg(b) if negb else b), negb


def _pair_want(a, nega, b, negb):
    """(kind, den as a field element or None, sum) from the points as handed over"""
    pa, pb = (T.g1_neg(a) if nega else a), (T.g1_neg(b) if negb else b)
    s = T.g1_add(pa, pb)
    if a is None and b is None:
        return 3, None, s
    if a is None:
        return 5, None, s
    if b is None:
        return 4, None, s
    if a[0] != b[0]:
        return 1, (b[0] - a[0]) % P, s
    if s is None:
        return 3, None, s
    return 2, 2 * pa[1] % P, s


def _pair_row(a, nega, b, negb, rng, extreme):
    return affine_digits(a, rng, extreme, 6, 6) + affine_digits(b, rng, extreme, 6, 6) + [nega, negb]


def t_pair_classify():
    def check(row, want, out):
        kind, den, _ = want
        if out[0] != kind:
            return "kind %s, expected %s" % (PAIR_NAMES.get(out[0], out[0]), PAIR_NAMES[kind])
        d = value(out[1:14])
        if (d - (1 if den is None else den) * RQ) % P:
            return "denominator %d" % d
        if not digits_ok(out[1:14], -BIG, BIG) or not abs(d) < 35 * P // 10:
            return "denominator outside the range of the zero test: %s" % out[1:14]
    t = Table("pair_classify", "pair_classify", 14, check)
    rng = random.Random(1208)
    for it in range(6 * 4 * 16):
        kind, nega, negb, extreme = KINDS[it % 6], (it // 6) & 1, (it // 12) & 1, bool((it // 24) & 1)
        a, b = operand_pair(kind, rng)
        # equal / opposite are meant as group elements after the signs: choose what is handed over accordingly
        a_in, b_in = (T.g1_neg(a) if nega else a), (T.g1_neg(b) if negb else b)
        t.add("%s nega=%d negb=%d" % (kind, nega, negb), _pair_row(a_in, nega, b_in, negb, rng, extreme),
              _pair_want(a_in, nega, b_in, negb))
    return t


def t_pair_batch():
    """pair_classify + fq_inv + pair_sum chained as the accumulation kernel does: one inversion per batch"""
    def check(row, want, out):
        kind, _, s = want
        if out[0] != kind:
            return "kind %s, expected %s" % (PAIR_NAMES.get(out[0], out[0]), PAIR_NAMES[kind])
        if kind not in (1, 2):
            return None if not any(out[1:]) else "a sum was written for kind %s" % PAIR_NAMES[kind]
        x3, y3 = value(out[1:14]), value(out[14:27])
        if (x3 * RQ_INV % P, y3 * RQ_INV % P) != s:
            return "sum (%x.., %x..), expected (%x.., %x..)" % (x3 * RQ_INV % P >> 320, y3 * RQ_INV % P >> 320, s[0] >> 320, s[1] >> 320)
        if not (digits_ok(out[1:14], -BIG, BIG) and digits_ok(out[14:27], -BIG, BIG)):
            return "digits above 2^29 + 4"
        if not (abs(x3) < 2 * P and abs(y3) < 13 * P // 10):
            return "magnitudes %.3f p, %.3f p" % (abs(x3) / P, abs(y3) / P)
    t = Table("pair_sum (shared inversion)", "pair_batch", 27, check, batches=[0])
    rng = random.Random(1209)
    plan = [("general",), ("equal",), ("opposite",), ("general", "equal"), ("equal", "b_inf"), None, None, None, None,
            ("opposite", "b_inf", "acc_inf", "both_inf", "opposite", "both_inf", "b_inf")]  # the last: nothing to invert
    sizes = [1, 1, 1, 2, 2, 7, 7, 64, 64, 7]
    for bi, (kinds, size) in enumerate(zip(plan, sizes)):
        for j in range(size):
            kind = kinds[j] if kinds else (KINDS[j % 6] if bi & 1 else rng.choice(KINDS))
            extreme = bool(j & 1)
            a, nega, b, negb = _pair_case(kind, rng, extreme)
            t.add(kind, _pair_row(a, nega, b, negb, rng, extreme), _pair_want(a, nega, b, negb), "batch %d of %d, slot %d" % (bi, size, j))
        t.batches.append(t.n)
    return t


# ---- wave compositions for the quad primitives -------------------------------------------------------------------------------
def wave_compositions():
    """[(name, [16 case kinds])]"""
    rng = random.Random(1301)
    waves = [("uniform " + k, [k] * 16) for k in KINDS]
    for idle in ("b_inf", "acc_inf"):
        for k in LIVE:
            for pos in (0, 7, 15):
                w = [idle] * 16
                w[pos] = k
                waves.append(("lone %s at %d, idle %s" % (k, pos, idle), w))
        for (p0, p1), (k0, k1) in (((0, 1), ("general", "equal")), ((3, 12), ("opposite", "general")), ((14, 15), ("general", "general"))):
            w = [idle] * 16
            w[p0], w[p1] = k0, k1
            waves.append(("two live (%s at %d, %s at %d), idle %s" % (k0, p0, k1, p1, idle), w))
    for other in ("equal", "opposite"):
        waves.append(("alternating %s / general" % other, [other if i % 2 == 0 else "general" for i in range(16)]))
        waves.append(("alternating general / %s" % other, ["general" if i % 2 == 0 else other for i in range(16)]))
    for i in range(32):
        waves.append(("random mixture %d" % i, [rng.choice(KINDS) for _ in range(16)]))
    return waves


_QUAD_CASES = []


def quad_cases():
    """[(kind, where, acc digits, b digits, acc point, b point)], built once and shared by every quad table"""
    if not _QUAD_CASES:
        rng = random.Random(1302)
        for wi, (name, kinds) in enumerate(wave_compositions()):
            for pos, kind in enumerate(kinds):
                extreme = bool((wi + pos) & 1)
                a, b = operand_pair(kind, rng)
                _QUAD_CASES.append((kind, "wave %d (%s), quad %d" % (wi, name, pos), xyzz_digits(a, rng, extreme),
                                    xyzz_digits(b, rng, extreme), a, b))
    return _QUAD_CASES


def _check_quad(row, want, out):
    """want: ('point', pt) or ('same', the 52 digits the accumulator must still hold)"""
    for q in range(1, 4):
        if out[q * 52:(q + 1) * 52] != out[:52]:
            return "lane %d of the quad differs from lane 0" % q
    if want[0] == "same":
        return None if out[:52] == want[1] else "a quad that made no call changed its accumulator"
    return check_xyzz(out[:52], want[1])


def _host_quad(run, table):
    rows = table.inputs()
    out = run("add", np.ascontiguousarray(rows[:, :104]), 52)
    skipped = rows[:, 104] == 0
    out[skipped] = rows[skipped, :52]
    return np.repeat(out, 4, axis=0).reshape(table.n, 4 * 52)


def t_add_quad(op, name, branch):
    """op: add_quad (every quad calls), add_quad_branch (only the quads with two finite operands call; word 104 says which)
    or add_quad_dense"""
    t = Table(name, op, 4 * 52, _check_quad, host=_host_quad)
    for kind, where, da, db, a, b in quad_cases():
        call = 1 if (not branch or kind in LIVE) else 0
        t.add(kind, da + db + [call], ("point", T.g1_add(a, b)) if call else ("same", da), where)
    return t


def _host_quad_loop(run, table):
    rows = table.inputs()
    acc = np.ascontiguousarray(rows[:, :52])
    for s in range(3):
        step = run("add", np.ascontiguousarray(np.concatenate([acc, rows[:, 52 * (1 + s):52 * (2 + s)]], axis=1)), 52)
        acc = np.where((rows[:, 208] > s)[:, None], step, acc)
    return np.repeat(acc, 4, axis=0).reshape(table.n, 4 * 52)


def t_add_quad_dense_loop():
    """the dense form inside a loop whose trip count (0..3) differs per quad: acc += the first `trip` of three operands"""
    t = Table("xyzz30_add_quad_dense in a loop", "add_quad_dense_loop", 4 * 52, _check_quad, host=_host_quad_loop)
    rng = random.Random(1303)
    for kind, where, da, db, a, b in quad_cases():
        trip = rng.choice((0, 1, 1, 2, 2, 3, 3))
        extra = [rng.choice((None, kG(rng.choice((-1, 1)) * rng.randrange(41, 60)))) for _ in range(2)]
        want = a
        for pt in ([b] + extra)[:trip]:
            want = T.g1_add(want, pt)
        row = da + db + [v for pt in extra for v in xyzz_digits(pt, rng, bool(trip & 1))] + [trip]
        t.add("%s trip=%d" % (kind, trip), row, ("point", want) if trip else ("same", da), where)
    return t


def t_quad_broadcast():
    """every lane holds its own value v; out[0..3] = fq_quad_broadcast<SRC>(v) - v for SRC = 0..3, digit-wise (the
    subtraction behind the move: what the DPP combiner folded); out[4..7] = broadcast<SRC + 1>(v) - broadcast<SRC>(v), the
    form P = U2 - U1 has in the cooperative addition"""
    def check(row, want, out):
        for j in range(8):
            if out[13 * j:13 * j + 13] != want[j]:
                what = "broadcast<%d>(v) - v" % j if j < 4 else "broadcast<%d>(v) - broadcast<%d>(v)" % ((j - 3) & 3, j - 4)
                return "%s = %s, expected %s" % (what, out[13 * j:13 * j + 13], want[j])
    t = Table("fq_quad_broadcast", "quad_broadcast", 104, check, host=False)
    rng = random.Random(1304)
    vals = [[rng.randrange(-(1 << 29), 1 << 29) for _ in range(13)] for _ in range(256)]
    for i, v in enumerate(vals):
        quad = vals[i & ~3:(i & ~3) + 4]
        want = [[x - y for x, y in zip(quad[src], v)] for src in range(4)]
        want += [[x - y for x, y in zip(quad[(src + 1) & 3], quad[src])] for src in range(4)]
        t.add("lane %d of its quad" % (i & 3), v, want, "wave %d quad %d" % (i // 64, (i % 64) // 4))
    return t


def t_quad_select():
    def check(row, want, out):
        if out != want:
            return "select = %s, expected %s" % (out, want)
    t = Table("fq_quad_select", "quad_select", 13, check, host=False)
    rng = random.Random(1305)
    for i in range(256):
        row = [rng.randrange(-(1 << 31), 1 << 31) for _ in range(52)]
        t.add("lane %d of its quad" % (i & 3), row, row[13 * (i & 3):13 * (i & 3) + 13])
    return t


# ---- the accumulation kernel's arithmetic: products that carry a third value, xyzz30_acc_* ---------------------------------------
# Everything below is modelled in integers: mont_py / mont_t give the exact integer of a reduction, so P, Rn and the whole
# tail are known digit for digit (a product's digits 0..11 are the balanced ones of its integer), and so is what
# fq_maybe_zero sees.
LOW = (1 << B) - 1
ZERO_RESIDUES = frozenset((k * P) & LOW for k in range(-3, 4))  # what digit 0 of k p can be, |k| <= 3
ONE = balanced(RQ % P)                                          # fq_one()
C_TOP = (1 << 31) - 4                                           # the largest digit of a raw sum of four: 4 (2^29 - 1)
ACC_KINDS = KINDS + ("false_positive",)
TAIL_KINDS = ("general", "false_positive")


def _c_variants(rng):
    """(name, digits) of the value taken into the carry pass: 0, raw sums of one to four normalised values, every digit at
    +-(2^31 - 4) with both signs of digit 12, -2^31 (four times -2^29), weakly normalised digits"""
    out = [("c=0", [0] * 13)]
    for n in (1, 2, 3, 4):
        parts = [balanced(_lazy(rng, 382)) for _ in range(n)]
        out.append(("c=raw sum of %d" % n, [sum(col) for col in zip(*parts)]))
    for s in (1, -1):
        for s12 in (1, -1):
            out.append(("c=%+d (2^31-4), digit 12 %+d 2^24" % (s, s12), [s * C_TOP] * 12 + [s12 << 24]))
    out.append(("c=+-(2^31-4)", [rng.choice((1, -1)) * C_TOP for _ in range(12)] + [rng.randrange(-(1 << 24), 1 << 24)]))
    out.append(("c=-2^31", [-(1 << 31)] * 12 + [1 << 24]))
    out.append(("c=+-(2^29+4)", [rng.choice((1, -1)) * BIG for _ in range(12)] + [rng.randrange(-(1 << 24), 1 << 24)]))
    return out


def _check_fused(row, want, out):
    """want: (the exact integer, the magnitude bound of field30.hip.h: 0.62 p + |a||b| / 2^390 + |c|)"""
    v = value(out)
    if v != want[0]:
        return "integer %d, expected %d (difference %d)" % (v, want[0], v - want[0])
    if not digits_ok(out):
        return "digits outside [-2^29, 2^29): %s" % out
    if not abs(v) < want[1]:
        return "magnitude %.3f p" % (v / P)


def _fused_want(a, b, c, sign):
    va, vb, vc = value(a), value(b), value(c)
    return mont_py(va, vb) + sign * vc, 62 * P // 100 + (abs(va * vb) >> 390) + abs(vc) + 1


def t_fq_mul_addc(sign):
    """fq_mul_minus (sign -1) / fq_mul_plus: exactly mont_py(a, b) -+ value(c).  Operands: the sets of fq_mul (adversarial sign
    patterns of the column bound with one operand a raw sum of two, raw sums, 2^385, 0, +-1, +-p), every adversarial pair with
    every form of c, the others with the forms of c in turn"""
    name = "fq_mul_minus" if sign < 0 else "fq_mul_plus"
    t = Table(name, name, 13, _check_fused)
    rng = random.Random(1401 if sign < 0 else 1402)
    cv = _c_variants(rng)
    for i, (kind, a, b) in enumerate(_field_operand_sets(rng, False)):
        for cname, c in (cv if kind == "adversarial" else [cv[i % len(cv)]]):
            t.add("%s %s" % (kind, cname), a + b + c, _fused_want(a, b, c, sign))
    return t


def t_fq_sqr_minus():
    """fq_sqr_minus: exactly mont_py(a, a) - value(c); a weakly normalised (the doubled operand of the square)"""
    t = Table("fq_sqr_minus", "fq_sqr_minus", 13, _check_fused)
    rng = random.Random(1403)
    cv = _c_variants(rng)
    n = 0
    for kind, a, b in _field_operand_sets(rng, True):
        for x in ((a,) if kind == "random" else (a, b)):
            for cname, c in (cv if kind == "adversarial" else [cv[n % len(cv)]]):
                t.add("%s %s" % (kind, cname), x + c, _fused_want(x, x, c, -1))
            n += 1
    return t


def maybe_zero_py(v):
    return 1 if (v & LOW) in ZERO_RESIDUES else 0


def t_fq_maybe_zero():
    """The one-word pre-test: true exactly when digit 0 is that of some k p, |k| <= 3, in whatever digits the value comes.
    True on a non-zero value is BY DESIGN (7 of the 2^30 residues: the near misses here, 7 x 2^-30 of all additions in the
    kernel): xyzz30_acc_rare runs the exact test behind it.  False must mean non-zero."""
    def check(row, want, out):
        if out[0] != want:
            return "maybe_zero = %d for %+.4f p, digit 0 %s that of a multiple of p" % (out[0], value(row) / P, "is" if want else "is not")
    t = Table("fq_maybe_zero", "fq_maybe_zero", 1, check)
    rng = random.Random(1404)

    def add(kind, d, expect):
        assert maybe_zero_py(value(d)) == expect, kind
        t.add(kind, d, expect)
    for k in range(-3, 4):
        d = balanced(k * P)
        add("%dp canonical" % k, d, 1)
        for j, up in ((0, 1), (0, -1), (11, 1), (5, -1)):
            e = list(d)
            e[j] += up << B
            e[j + 1] -= up
            add("%dp re-split at digit %d" % (k, j), e, 1)
        for _ in range(8):
            u = _lazy(rng, 382)
            raw = [x - y for x, y in zip(balanced(u), balanced(u - k * P))]
            assert value(raw) == k * P
            add("%dp raw difference" % k, raw, 1)
            add("%dp norm(raw difference)" % k, _weak(raw), 1)
        for _ in range(16):  # the false positives: digit 0 of k p, another integer
            v = k * P + rng.choice((-1, 1)) * rng.randrange(1, 1 << 350) * (1 << B)
            assert v % P
            add("near miss of %dp" % k, balanced(v), 1)
        for off in (1, -1, 1 << 29, rng.randrange(2, 1 << 29)):
            add("%dp + %d" % (k, off), balanced(k * P + off), 0)
    for k in (-5, -4, 4, 5):
        add("%dp" % k, balanced(k * P), 0)
    for _ in range(512):
        v = rng.randrange(-35 * P // 10 + 1, 35 * P // 10)
        t.add("random", balanced(v), maybe_zero_py(v))
    return t


# ---- xyzz30_acc_*: operands ---------------------------------------------------------------------------------------------------
def raw_two(d, rng, extreme):
    """the integer of the balanced digits d in the digits X has inside the kernel: a raw sum W + Q of two normalised values,
    each digit 0..11 in [-2^30, 2^30 - 2].  A digit is re-split to the far side of zero (extreme: wherever it can be)"""
    out = list(d)
    for i in range(12):
        if not (extreme or rng.randrange(2)):
            continue
        s = -1 if out[i] >= 0 else 1
        cand = out[i] + s * (1 << B)
        if -(1 << B) <= cand <= (1 << B) - 2:
            out[i] = cand
            out[i + 1] -= s
    assert value(out) == value(d) and digits_ok(out, -(1 << B), (1 << B) - 2), out
    return out


def _sqrt(v):
    """a square root mod p (p = 3 mod 4), or None"""
    s = pow(v, (P + 1) // 4, P)
    return s if s * s % P == v % P else None


def _acc_from_z(a, z, rng, extreme, raw_x, X=None):
    zz, zzz = z * z % P, z * z * z % P
    d = (rep(a[0] * zz % P, 26, rng, extreme) if X is None else X) + rep(a[1] * zzz % P, 13, rng, extreme) + \
        rep(zz, 7, rng, extreme) + rep(zzz, 7, rng, extreme)
    if raw_x and X is None:
        d[:13] = raw_two(d[:13], rng, extreme)
    return d


def false_positive_row(rng, neg, extreme, raw_x):
    """An addition of two different points whose P = U2 - X1 passes the one-word pre-test: t = 0 (mod 2^30) in [1, p),
    ZZ = t / ((x_b - x_a) 2^390) where that is a square, so that P = t + k p; |P| < 3.3 p leaves k in -4 .. 3 and every k
    but -4 is one of the seven residues.  Drawn again until it is; nothing is skipped.  -> (row, a, b)"""
    while True:
        a, b = operand_pair("general", rng)
        t = rng.randrange(1, P >> B) << B
        z = _sqrt(t * pow((b[0] - a[0]) * RQ, -1, P) % P)
        if z is None:
            continue
        row = _acc_from_z(a, z, rng, extreme, raw_x) + affine_digits(T.g1_neg(b) if neg else b, rng, extreme) + [neg]
        code, Pv, _ = head_py(row)
        assert (Pv - t) % P == 0 and Pv % P != 0 and abs(Pv) < 33 * P // 10
        if code != 4:
            assert Pv == t - 4 * P
            continue
        return row, a, b


def adversarial_x_row(kind, rng, sign, neg):
    """An accumulator whose X has EVERY digit 0..11 at the end of the raw sum's range (-2^30 or 2^30 - 2; digit 12 free below
    2.6 p): ZZ = X / (x_a 2^390) where that is a square.  Squared without the carry pass of xyzz30_acc_settle such an X
    overflows the column bound (6 x 2^61 + 2^60 > 2^63), with it nothing does.  -> (row, a, b)"""
    top = (26 * P // 10) >> 360
    while True:
        a, b = operand_pair(kind, rng)
        X = [-(1 << B) if sign < 0 else (1 << B) - 2] * 12 + [rng.randrange(-top + 2, top - 1)]
        assert abs(value(X)) < 26 * P // 10
        z = _sqrt(value(X) * pow(a[0] * RQ, -1, P) % P)
        if z is None:
            continue
        return _acc_from_z(a, z, rng, True, True, X) + affine_digits(T.g1_neg(b) if neg else b, rng, True) + [neg], a, b


def acc_row(kind, rng, neg, extreme, raw_x):
    """(79 ints: accumulator, point as handed over, neg; the accumulator's point; the point added)"""
    if kind == "false_positive":
        return false_positive_row(rng, neg, extreme, raw_x)
    a, b = operand_pair(kind, rng)
    acc = xyzz_digits(a, rng, extreme)
    if raw_x and a is not None:
        acc[:13] = raw_two(acc[:13], rng, extreme)
    return acc + affine_digits(T.g1_neg(b) if neg else b, rng, extreme) + [neg], a, b


# ---- xyzz30_acc_*: the integers of the same formulas ------------------------------------------------------------------------------
def head_py(row):
    """(code, P, Rn) of xyzz30_acc_head as integers: P = x2 ZZ - X, Rn = (-y2) ZZZ + Y with y2 negated when neg"""
    X, Y, ZZ, ZZZ, px, py = (value(row[13 * j:13 * j + 13]) for j in range(6))
    Pv = mont_py(px, ZZ) - X
    Rn = mont_py(py if row[78] else -py, ZZZ) + Y
    code = (0 if any(row[52:78]) else 1) | (0 if any(row[26:39]) else 2) | (4 if maybe_zero_py(Pv) else 0)
    return code, Pv, Rn


def tail_py(acc, Pv, Rn):
    """the 52 digits xyzz30_acc_tail leaves: X = W + Q digit-wise, Y, ZZ, ZZZ straight from a product"""
    X, Y, ZZ, ZZZ = (value(acc[13 * j:13 * j + 13]) for j in range(4))
    PP = mont_py(Pv, Pv)
    ZZ3 = mont_py(ZZ, PP)
    Q = mont_py(X, PP)
    PPP = mont_py(Pv, PP)
    ZZZ3 = mont_py(ZZZ, PPP)
    W = mont_py(Rn, Rn) - (PPP + 3 * Q)
    Y3 = mont_t(Rn * W - Y * PPP)
    return [w + q for w, q in zip(balanced(W), balanced(Q))] + balanced(Y3) + balanced(ZZ3) + balanced(ZZZ3)


def check_acc_inside(out, want, tail_ran):
    """the accumulator as it stays inside k_bucket_accumulate (g1_30.hip.h): the point, ZZ^3 = ZZZ^2, the magnitude line,
    digits of X in [-2^30, 2^30).  Y, ZZ and ZZZ: straight from a product (digits in [-2^29, 2^29)) when the tail ran;
    a doubling leaves Y behind a carry pass, a first point or an untouched accumulator is what came in (<= 2^29 + 4)"""
    if want is None:
        return None if not any(out) else "expected infinity as exact zeros, got %s" % out
    X, Y, ZZ, ZZZ = (value(out[13 * i:13 * i + 13]) for i in range(4))
    if ZZ % P == 0 or ZZZ % P == 0:
        return "ZZ or ZZZ is zero mod p for a finite sum"
    got = (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P)
    if got != want:
        return "point (%x.., %x..), expected (%x.., %x..)" % (got[0] >> 320, got[1] >> 320, want[0] >> 320, want[1] >> 320)
    if pow(ZZ * RQ_INV, 3, P) != pow(ZZZ * RQ_INV, 2, P):
        return "ZZ^3 != ZZZ^2"
    if not digits_ok(out[:13], -(1 << B), (1 << B) - 1):
        return "digits of X outside [-2^30, 2^30): %s" % out[:13]
    for i in (1, 2, 3):
        d = out[13 * i:13 * i + 13]
        if not (digits_ok(d) if tail_ran else digits_ok(d, -BIG, BIG)):
            return "digits of coordinate %d outside %s: %s" % (i, "[-2^29, 2^29)" if tail_ran else "+-(2^29 + 4)", d)
    for name, v, m10 in (("X", X, 26), ("Y", Y, 13), ("ZZ", ZZ, 7), ("ZZZ", ZZZ, 7)):
        if not abs(v) < m10 * P // 10:
            return "|%s| = %.3f p, stated bound %.1f p" % (name, abs(v) / P, m10 / 10)


def _check_acc_madd(row, want, out):
    """want: (the sum, whether xyzz30_acc_tail produces it).  Unsettled: check_acc_inside; settled: check_xyzz as it is,
    the same Y, ZZ, ZZZ and one carry pass on X"""
    pt, tail_ran = want
    msg = check_acc_inside(out[:52], pt, tail_ran)
    if msg:
        return "inside the kernel: " + msg
    msg = check_xyzz(out[52:], pt)
    if msg:
        return "settled: " + msg
    if out[65:] != out[13:52] or out[52:65] != norm_py(out[:13]):
        return "settled is not one carry pass on X and nothing else"


_ACC_CASES = {}


def acc_cases():
    """[(kind, row, a, b)]: the six KINDS of t_madd and the constructed false positives x neg x extreme / random
    representatives x X balanced / X as the kernel holds it (a raw sum of two), then X at the ends of the raw sum's range.
    Built once, shared by the tables of the head, the rare call, the tail and the whole addition."""
    if not _ACC_CASES:
        rng = random.Random(1405)
        cases = []
        for it in range(7 * 8 * 12):
            kind, neg, extreme, raw_x = ACC_KINDS[it % 7], (it // 7) & 1, bool((it // 14) & 1), bool((it // 28) & 1)
            row, a, b = acc_row(kind, rng, neg, extreme, raw_x)
            cases.append(("%s neg=%d %s X %s" % (kind, neg, "extreme" if extreme else "random", "raw" if raw_x else "balanced"), row, a, b))
        for kind in LIVE:
            for sign in (1, -1):
                for neg in (0, 1):
                    row, a, b = adversarial_x_row(kind, rng, sign, neg)
                    cases.append(("%s neg=%d extreme X raw, every digit %s" % (kind, neg, "2^30 - 2" if sign > 0 else "-2^30"), row, a, b))
        _ACC_CASES["all"] = cases
    return _ACC_CASES["all"]


def t_acc_madd():
    t = Table("xyzz30_acc_madd", "acc_madd", 104, _check_acc_madd)
    for kind, row, a, b in acc_cases():
        t.add(kind, row, (T.g1_add(a, b), kind.startswith(TAIL_KINDS)))
    return t


def t_acc_head():
    def check(row, want, out):
        if out[0] != want[0]:
            return "code %d, expected %d" % (out[0], want[0])
        if out[1:14] != want[1]:
            return "P = %s, expected %s" % (out[1:14], want[1])
        if out[14:27] != want[2]:
            return "Rn = %s, expected %s" % (out[14:27], want[2])
    t = Table("xyzz30_acc_head", "acc_head", 27, check)
    for kind, row, a, b in acc_cases():
        code, Pv, Rn = head_py(row)
        # what the case kinds promise, from the integers
        if kind.startswith("false_positive"):
            assert code == 4 and Pv % P != 0, kind
        if kind.startswith(("equal", "opposite")):
            assert code == 4 and Pv % P == 0 and (Rn % P == 0) == kind.startswith("equal"), kind
        if kind.startswith("general"):
            assert code in (0, 4) and Pv % P != 0, kind
        t.add(kind, row, (code, balanced(Pv), balanced(Rn)))
    return t


def t_acc_rare():
    """acc, P, Rn as the head leaves them, for every case that enters the call: a false positive comes back untouched with
    `true`, equal operands doubled (behind the carry pass on X) and opposite ones as infinity with `false`"""
    def check(row, want, out):
        flag, pt = want
        if out[0] != flag:
            return "returned %d, expected %d" % (out[0], flag)
        if flag:
            return None if out[1:] == row[:52] else "a false positive changed the accumulator"
        return check_xyzz(out[1:], pt)
    t = Table("xyzz30_acc_rare", "acc_rare", 53, check)
    for kind, row, a, b in acc_cases():
        code, Pv, Rn = head_py(row)
        if code != 4:
            continue
        if Pv % P:
            want = (1, None)
        else:
            want = (0, T.g1_add(a, a) if Rn % P == 0 else None)
        t.add(kind, row[:52] + balanced(Pv) + balanced(Rn), want)
    return t


def t_acc_tail():
    """acc, P, Rn as the head leaves them for two different points: the digits of the same formulas on integers"""
    def check(row, want, out):
        digits, pt = want
        if out != digits:
            j = next(i for i in range(52) if out[i] != digits[i])
            return "%s digit %d is %d, the integers give %d" % ("X Y ZZ ZZZ".split()[j // 13], j % 13, out[j], digits[j])
        return check_acc_inside(out, pt, True)
    t = Table("xyzz30_acc_tail", "acc_tail", 52, check)
    for kind, row, a, b in acc_cases():
        if not kind.startswith(TAIL_KINDS):
            continue
        _, Pv, Rn = head_py(row)
        t.add(kind, row[:52] + balanced(Pv) + balanced(Rn), (tail_py(row[:52], Pv, Rn), T.g1_add(a, b)))
    return t


def acc_zero_multiples(table):
    """For the equal / opposite cases of a table of (acc, point, neg) rows: which multiples of p their P = U2 - X1 and
    Rn = Y1 - S2 are, {"P": {k: first case}, "R": {k: first case}} (R = -Rn), and how many false positives it holds"""
    seen = {"P": {}, "R": {}, "false_positive": 0}
    for i, row in enumerate(table.rows):
        code, Pv, Rn = head_py(row)
        if table.kinds[i].startswith("false_positive"):
            assert code == 4 and Pv % P != 0
            seen["false_positive"] += 1
        if not table.kinds[i].startswith(("equal", "opposite")):
            continue
        assert Pv % P == 0
        seen["P"].setdefault(Pv // P, i)
        if Rn % P == 0:
            seen["R"].setdefault(-Rn // P, i)
    return seen


# ---- chains: the unsettled accumulator feeds the next step, a constructed false positive at step 7 ---------------------------------
FP_STEP = 7


def _curve_point_for(acc, rng):
    """a curve point b (of E(Fp): the formulas do not ask for the subgroup) whose addition to the accumulator with the digits
    `acc` passes the pre-test without being equal or opposite: x_b = (t + X) / ZZ for t = 0 (mod 2^30)"""
    X, ZZ = value(acc[:13]), value(acc[26:39])
    while True:
        t = rng.randrange(1, P >> B) << B
        x = (t + X) * pow(ZZ, -1, P) % P
        y = _sqrt(x * x * x + 4)
        if y is not None:
            return (x, y if rng.randrange(2) else P - y)


def t_chain_acc_madd():
    """chain_points with step 7 replaced: steps 0..3 are P, P, -2P, infinity; step 4 sets the accumulator from a point
    (ZZ = ZZZ = fq_one()), step 5 adds infinity, step 6 a general point -- from there the accumulator is known digit for
    digit (tail_py) -- and step 7 is a curve point built against those digits so that the pre-test fires on P != 0.
    want: (the 16 partial sums, the settled digits after step 6)"""
    def check(row, want, out):
        partial, model = want
        for s in range(16):
            rec = out[s * 52:(s + 1) * 52]
            msg = check_xyzz(rec, partial[s])
            if msg:
                return "step %d: %s" % (s, msg)
            if s == FP_STEP - 1 and rec != model:
                return "step %d: the accumulator in front of the false positive is not the one the integers give" % s
    t = Table("chain xyzz30_acc_madd", "chain_acc_madd", 16 * 52, check)
    rng = random.Random(1406)
    for it in range(64):
        extreme = bool(it & 1)
        while True:
            seq, _ = chain_points(rng)
            if seq[4][0] != seq[6][0]:
                break
        negs = [rng.randrange(2) for _ in range(16)]
        steps = [affine_digits(T.g1_neg(pt) if neg else pt, rng, extreme) + [neg] for pt, neg in zip(seq, negs)]
        acc = steps[4][:13] + [(-v if negs[4] else v) for v in steps[4][13:26]] + ONE + ONE   # xyzz30_acc_set
        code, Pv, Rn = head_py(acc + steps[6])
        assert code == 0
        acc = tail_py(acc, Pv, Rn)
        while True:
            b = _curve_point_for(acc, rng)
            step = affine_digits(T.g1_neg(b) if negs[FP_STEP] else b, rng, extreme) + [negs[FP_STEP]]
            code, Pv, _ = head_py(acc + step)
            assert Pv % P != 0
            if code == 4:
                break
        seq[FP_STEP], steps[FP_STEP] = b, step
        partial, s = [], None
        for pt in seq:
            s = T.g1_add(s, pt)
            partial.append(s)
        t.add("chain %s" % ("extreme" if extreme else "random"), [v for st in steps for v in st],
              (partial, norm_py(acc[:13]) + acc[13:]))
    return t


# ---- one step of the kernel's dispatch: whole waves of chosen lane kinds -------------------------------------------------------------
# general; fresh (acc_inf); fresh with the point at infinity (both_inf); the point at infinity on a finite accumulator
# (b_inf); equal; opposite; false positive
LANE_KINDS = ("general", "acc_inf", "both_inf", "b_inf", "equal", "opposite", "false_positive")
RARE_LANES = LANE_KINDS[1:]


def dispatch_waves():
    """[(name, [64 lane kinds])]: uniform waves, one lane of each rare kind among general lanes, every kind in one wave,
    random mixtures"""
    rng = random.Random(1407)
    waves = [("uniform " + k, [k] * 64) for k in LANE_KINDS]
    for k in RARE_LANES:
        for pos in (0, 37, 63):
            w = ["general"] * 64
            w[pos] = k
            waves.append(("lone %s at lane %d" % (k, pos), w))
    waves.append(("every kind in turn", [LANE_KINDS[i % 7] for i in range(64)]))
    w = [LANE_KINDS[i % 7] for i in range(64)]
    rng.shuffle(w)
    waves.append(("every kind shuffled", w))
    for i in range(8):
        waves.append(("random mixture %d" % i, [rng.choice(LANE_KINDS) for _ in range(64)]))
    return waves


def _host_dispatch(run, table):
    return run("acc_madd", table.inputs(), 104)


def t_acc_dispatch():
    """every lane's result is the single-lane expectation of xyzz30_acc_madd, whatever the other lanes of its wave do"""
    t = Table("dispatch of k_bucket_accumulate (ballot, second read, call through private memory, tail)", "acc_dispatch", 104,
              _check_acc_madd, host=_host_dispatch)
    rng = random.Random(1408)
    for wi, (name, kinds) in enumerate(dispatch_waves()):
        for lane, kind in enumerate(kinds):
            neg, extreme, raw_x = rng.randrange(2), bool((wi + lane) & 1), bool(((wi + lane) >> 1) & 1)
            row, a, b = acc_row(kind, rng, neg, extreme, raw_x)
            t.add(kind, row, (T.g1_add(a, b), kind in TAIL_KINDS), "wave %d (%s), lane %d" % (wi, name, lane))
    return t


# ---- the tables ----------------------------------------------------------------------------------------------------------------------
FAMILIES = {
    "fp_products": (t_fq_mul, t_fq_sqr, t_fq_mul_sub),
    "fp_carries_and_signs": (t_fq_norm, t_fq_norm_wide, t_fq_neg_plain, t_fq_neg, t_fq_canon_digits),
    "fp_zero_test": (t_fq_is_zero,),
    "fp_storage_and_canonical_form": (t_fq_from_u32x12, t_fq_to_u32x12, t_fq_canon_half),
    "fp_inverse": (t_fq_inv,),
    "fr": (t_fr30_mul, t_fr30_norm, t_fr30_from_limbs, t_fr30_to_limbs, t_fr30_abs_to_limbs, t_fr30_inv),
    "group_law_one_lane": (t_madd, t_add, t_add_call, t_dbl),
    "group_law_chains": (t_chain_madd, t_chain_add, lambda: t_chain_quad(False), lambda: t_chain_quad(True)),
    "affine_pairs": (t_pair_classify, t_pair_batch),
    "quad_sparse": (lambda: t_add_quad("add_quad", "xyzz30_add_quad, every quad calls", False),
                    lambda: t_add_quad("add_quad_branch", "xyzz30_add_quad behind a branch on the quad", True)),
    "quad_dense": (lambda: t_add_quad("add_quad_dense", "xyzz30_add_quad_dense", False), t_add_quad_dense_loop),
    "quad_moves": (t_quad_broadcast, t_quad_select),
    "accum_fused_products": (lambda: t_fq_mul_addc(-1), lambda: t_fq_mul_addc(1), t_fq_sqr_minus, t_fq_maybe_zero),
    "accum_mixed_addition": (t_acc_head, t_acc_rare, t_acc_tail, t_acc_madd, t_chain_acc_madd, t_acc_dispatch),
}
FR_OPS = ("fr30_mul", "fr30_norm", "fr30_from_limbs", "fr30_to_limbs", "fr30_abs_to_limbs", "fr30_inv")
_BUILT = {}


def family(name):
    """the tables of one family, built once per process"""
    if name not in _BUILT:
        _BUILT[name] = [make() for make in FAMILIES[name]]
    return _BUILT[name]


# ---- what the zero tests of xyzz30_madd meet -----------------------------------------------------------------------------------
def madd_zero_multiples(table):
    """For the equal / opposite cases of the xyzz30_madd table: which multiples of p its P = U2 - X1 and R = S2 - Y1 are, as
    {"P": {k: first case index}, "R": {...}}, with the products taken by mont_py (the exact integer the multiplier returns)."""
    seen = {"P": {}, "R": {}}
    for i, row in enumerate(table.rows):
        if not table.kinds[i].startswith(("equal", "opposite")):
            continue
        X, Y, ZZ, ZZZ, px, py = (value(row[13 * j:13 * j + 13]) for j in range(6))
        if row[78]:
            py = -py
        Pv = mont_py(px, ZZ) - X
        Rv = mont_py(py, ZZZ) - Y
        assert Pv % P == 0
        seen["P"].setdefault(Pv // P, i)
        if Rv % P == 0:
            seen["R"].setdefault(Rv // P, i)
    return seen
