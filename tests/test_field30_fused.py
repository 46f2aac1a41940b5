"""Host-side checks of the accumulation kernel's fused arithmetic against Python big integers: fq_mul_minus / fq_mul_plus /
fq_sqr_minus (csrc/field30.hip.h: a product that subtracts or adds a third value inside its own carry pass) and the mixed
addition built on them (xyzz30_acc_*, csrc/g1_30.hip.h) against the unfused xyzz30_madd and textbook affine arithmetic.
CPU only: the headers are __host__ __device__ code, compiled here with g++ (tests/host/field30_fused_host.cpp)."""
import ctypes
import os
import random
import subprocess

import pytest

import accum_false_positives as FP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
B, N = 30, 13
RQ = 1 << 390
I13 = ctypes.c_int32 * 13
I52 = ctypes.c_int32 * 52
BIG = (1 << 29) + 4
GX = 0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb
GY = 0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("f30f") / "libf30f.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "host", "field30_fused_host.cpp")],
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
    assert -(1 << 31) <= v < (1 << 31)
    return d


def value(d):
    return sum(int(x) << (B * i) for i, x in enumerate(d))


def call3(fn, a, b, c):
    r = I13()
    fn(I13(*a), I13(*b), I13(*c), r)
    return list(r)


def call2(fn, a, c):
    r = I13()
    fn(I13(*a), I13(*c), r)
    return list(r)


def strict(r):
    return all(-(1 << 29) <= x < (1 << 29) for x in r[:12])


def check_product(lib, a, b, c):
    """a, b, c: digit lists.  The fused results are the plain product's integer -+ c's integer, exactly, the plain product is
    a b / 2^390 (mod p), and digits 0..11 are exactly balanced."""
    va, vb, vc = value(a), value(b), value(c)
    ref = call2(lib.f30f_mul, a, b)
    assert (value(ref) * RQ - va * vb) % P == 0
    m = call3(lib.f30f_mul_minus, a, b, c)
    assert value(m) == value(ref) - vc
    assert ((value(m) + vc) * RQ - va * vb) % P == 0
    assert strict(m)
    assert abs(value(m)) < 0.62 * P + (abs(va) * abs(vb) >> 390) + abs(vc) + 1
    s = call3(lib.f30f_mul_plus, a, b, c)
    assert value(s) == value(ref) + vc
    assert strict(s)


def check_square(lib, a, c):
    va, vc = value(a), value(c)
    r = I13()
    lib.f30f_sqr(I13(*a), r)
    ref = list(r)
    assert (value(ref) * RQ - va * va) % P == 0
    m = call2(lib.f30f_sqr_minus, a, c)
    assert value(m) == value(ref) - vc
    assert ((value(m) + vc) * RQ - va * va) % P == 0
    assert strict(m)


def max_column(a, b, c):
    """largest |column| of fq_mul_minus in exact arithmetic, sum of magnitudes (the worst sign pattern), carry-in included"""
    pd = balanced(P)
    worst = 0
    for k in range(25):
        mag = 1 << 34
        for i in range(13):
            j = k - i
            if 0 <= j <= 12:
                mag += abs(a[i] * b[j]) + (1 << 29) * abs(pd[j])
        if k >= 13:
            mag += abs(c[k - 13])
        worst = max(worst, mag)
    return worst


def test_fused_products_random(lib):
    rng = random.Random(1601)
    for it in range(2000):
        a, b, c = (balanced(rng.randrange(-(1 << 383), 1 << 383)) for _ in range(3))
        check_product(lib, a, b, c)
        check_square(lib, a, c)


def test_fused_products_at_the_contract_edges(lib):
    rng = random.Random(1602)
    sign = lambda: rng.choice((1, -1))  # noqa: E731
    top = lambda: rng.randrange(-(1 << 24), 1 << 24)  # noqa: E731
    for it in range(300):
        # every digit at +-(2^29 + 4)
        a = [sign() * BIG for _ in range(12)] + [top()]
        b = [sign() * BIG for _ in range(12)] + [top()]
        c = [sign() * BIG for _ in range(12)] + [top()]
        check_product(lib, a, b, c)
        check_square(lib, a, c)
        # c a raw sum of four normalised values: digits down to -2^31 and up to 4 (2^29 - 1)
        c4 = [rng.choice((4 * ((1 << 29) - 1), -4 * (1 << 29))) for _ in range(12)] + [4 * top()]
        check_product(lib, a, b, c4)
        check_square(lib, a, c4)
        assert max_column(a, b, c4) < 1 << 63
        # one multiplicand a raw sum of two
        a2 = [sign() * 2 * BIG for _ in range(12)] + [2 * top()]
        bs = [sign() * (1 << 29) for _ in range(12)] + [top()]  # 2 (2^29 + 4) x 2^29 <= 2.1 x 2^58
        check_product(lib, a2, bs, c4)
        assert max_column(a2, bs, c4) < 1 << 63
    # same signs everywhere, and the sign pattern of p's own digits (maximises the m p part)
    pd = balanced(P)
    for sa in (1, -1):
        for sc in (1, -1):
            a = [sa * BIG] * 12 + [1 << 24]
            b = [BIG] * 12 + [1 << 24]
            c = [sc * 4 * ((1 << 29) - 1)] * 12 + [sc << 26]
            check_product(lib, a, b, c)
            check_square(lib, a, c)
            ap = [sa * (BIG if x >= 0 else -BIG) for x in pd[:12]] + [0]
            check_product(lib, ap, b, c)
            assert max_column(ap, b, c) < 1 << 63


def test_fused_products_at_the_group_laws_magnitudes(lib):
    """values at the p-multiples stated in g1_30.hip.h: P = x2 ZZ - X with X = +-2.6 p, Rn = (-y2) ZZZ + Y with Y = +-1.3 p,
    W = Rn^2 - (PPP + 3 Q) with |Rn| = 2 p and |PPP|, |Q| = 0.63 p"""
    rng = random.Random(1603)
    near = lambda k: int(k * P) + rng.randrange(-(1 << 300), 1 << 300)  # noqa: E731
    for it in range(200):
        s1, s2, s3 = (rng.choice((1, -1)) for _ in range(3))
        x2, zz, X = balanced(near(0.62 * s1)), balanced(near(0.7 * s2)), near(2.6 * s3)
        wv = near(1.9 * s3)
        w, q = balanced(wv), balanced(X - wv)
        Xraw = [u + v for u, v in zip(w, q)]  # X as the kernel keeps it: a raw sum of two
        check_product(lib, x2, zz, Xraw)
        Pv = value(call3(lib.f30f_mul_minus, x2, zz, Xraw))
        assert abs(Pv) < 3.3 * P
        y2, zzz, Y = balanced(near(0.62 * s1)), balanced(near(0.7 * s2)), balanced(near(1.3 * s3))
        check_product(lib, y2, zzz, Y)
        assert abs(value(call3(lib.f30f_mul_plus, y2, zzz, Y))) < 2 * P
        rn, ppp, qq = balanced(near(2.0 * s1)), balanced(near(0.63 * s2)), balanced(near(0.63 * s2))
        c4 = [u + 3 * v for u, v in zip(ppp, qq)]
        check_square(lib, rn, c4)
        assert abs(value(call2(lib.f30f_sqr_minus, rn, c4))) < 3.2 * P


def test_maybe_zero_is_the_pre_test_of_is_zero(lib):
    rng = random.Random(1604)
    for k in range(-3, 4):
        d = balanced(k * P)
        d[3] += 1 << 30
        d[4] -= 1
        assert lib.f30f_maybe_zero(I13(*d)) == 1
    hits = sum(lib.f30f_maybe_zero(I13(*balanced(rng.randrange(-3 * P, 3 * P)))) for _ in range(2000))
    assert hits <= 2  # seven residues out of 2^30


# ---- group law ---------------------------------------------------------------------------------------------------------
def ec_add(p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def affine_digits(pt):
    # mixes negative and positive representatives of x
    return balanced((pt[0] * RQ) % P - (P if pt[0] & 1 else 0)), balanced((pt[1] * RQ) % P)


def affine_of(acc):
    X, Y, ZZ, ZZZ = (value(list(acc)[13 * k:13 * k + 13]) for k in range(4))
    if ZZ == 0:
        assert all(v == 0 for v in list(acc))  # infinity is only ever written as exact zeros
        return None
    assert ZZ % P != 0
    rinv = pow(RQ, -1, P)
    assert (ZZ * rinv) ** 3 % P == (ZZZ * rinv) ** 2 % P
    return X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P


def check_bounds(acc):
    """the digit and magnitude bounds written in g1_30.hip.h for an accumulator inside the kernel"""
    d = list(acc)
    X, Y, ZZ, ZZZ = (d[13 * k:13 * k + 13] for k in range(4))
    assert all(-(1 << 30) <= x < (1 << 30) for x in X[:12])  # a raw sum of two (2^30 + 8 would still be inside fq_mul's contract)
    for f in (Y, ZZ, ZZZ):
        assert all(abs(x) <= BIG for x in f[:12])
    for f, bound in ((X, 2.6), (Y, 1.3), (ZZ, 0.7), (ZZZ, 0.7)):
        assert abs(value(f)) < bound * P


@pytest.fixture(scope="module")
def multiples():
    pts = [(GX, GY)]
    for _ in range(11):
        pts.append(ec_add(pts[-1], (GX, GY)))  # G .. 12 G (G has odd prime order: no 2-torsion anywhere)
    return pts


def run_script(lib, pts, script, acc_new=None, acc_old=None, want=None):
    acc_new = acc_new or I52()
    acc_old = acc_old or I52()
    for idx, neg in script:
        if idx is None:
            px, py, q = [0] * 13, [0] * 13, None  # the point at infinity
        else:
            px, py = affine_digits(pts[idx])
            q = pts[idx] if not neg else (pts[idx][0], (-pts[idx][1]) % P)
        lib.f30f_acc_madd(acc_new, I13(*px), I13(*py), neg)
        lib.f30f_madd(acc_old, I13(*px), I13(*py), neg)
        want = ec_add(want, q)
        assert affine_of(acc_new) == want, (idx, neg)
        assert affine_of(acc_old) == want
        assert lib.f30f_same_point(acc_new, acc_old) == 1
        check_bounds(acc_new)
    return acc_new, acc_old, want


def test_fused_mixed_addition_complete_cases(lib, multiples):
    """accumulator at infinity, point at infinity, P + P (doubling of a 2-torsion-free point), P - P, and passing through
    infinity and out again"""
    script = [(None, 0),                  # infinity + infinity
              (0, 0),                     # accumulator at infinity
              (None, 1),                  # point at infinity
              (0, 0),                     # G + G: doubling
              (1, 1), (1, 0),             # 2G - 2G = infinity, then 2G again
              (1, 0),                     # 2G + 2G: doubling of an accumulator set from a point
              (3, 1),                     # 4G - 4G
              (5, 0), (2, 0), (7, 0), (7, 1), (2, 1), (5, 1),  # up and back down to infinity through a cancellation
              (4, 1), (4, 1), (9, 0)]     # -5G - 5G: doubling with a negated point; -10G + 10G
    run_script(lib, multiples, script)


def test_fused_mixed_addition_random_chains(lib, multiples):
    """chains of 200 additions of random signed multiples of G (doublings and cancellations occur on their own as well);
    the flushed form: one carry pass on X, then the readers of a flushed accumulator (the general addition, doubling
    branch included, which squares X)"""
    rng = random.Random(1605)
    ends = []
    for chain in range(3):
        script = [(rng.randrange(12), rng.randrange(2)) for _ in range(200)]
        acc_new, acc_old, want = run_script(lib, multiples, script)
        before = list(acc_new)
        lib.f30f_acc_settle(acc_new)
        after = list(acc_new)
        assert value(after[:13]) == value(before[:13]) and after[13:] == before[13:]
        assert all(abs(x) <= BIG for x in after[:12])
        ends.append((acc_new, acc_old, want))
    for (a_new, a_old, wa), (b_new, _, wb) in ((ends[0], ends[1]), (ends[1], ends[2]), (ends[2], ends[2])):
        s = I52(*list(a_new))
        lib.f30f_add(s, b_new)  # the last pair: equal operands
        assert affine_of(s) == ec_add(wa, wb)
        s = I52(*list(a_new))
        lib.f30f_add(s, a_old)  # equal group elements in different representations
        assert affine_of(s) == ec_add(wa, wa)


# ---- the pre-test's false positives on a real SRS (accum_false_positives.py) ---------------------------------------------
@pytest.fixture(scope="module")
def rows_kg():
    return FP.multiples_of_g(FP.N_ROWS)


def test_table_digits_of_loaded_rows(lib, rows_kg):
    """f30f_table_digits: x 2^390 (mod p) below 0.62 p in exactly balanced digits, from blst's words of x"""
    pts = rows_kg[:64] + rows_kg[-64:]
    dig = FP.table_digits(lib, FP.affine_rows(pts))
    for pt, d in zip(pts, dig.tolist()):
        for c, dd in zip(pt, (d[:13], d[13:])):
            assert (value(dd) - c * RQ) % P == 0 and abs(value(dd)) < 0.62 * P and strict(dd)


def test_false_positive_pairs_among_the_rows_kG(lib, rows_kg):
    """On the rows k G, k = 1 .. 65537, the host model of "set a, then head b" finds unordered pairs of DIFFERENT points whose
    P = U2 - X1 passes the one-word zero pre-test in both orders of arrival (measured: 11).  The GPU test of
    k_bucket_accumulate (tests/test_accum_false_positive_gpu.py) puts exactly these pairs into buckets of two.  Fewer
    than four is a failure, never a skip.  The fused addition gives (k_i + k_j) G for each, through the false-positive return
    of xyzz30_acc_rare."""
    assert rows_kg[1] == ec_add(rows_kg[0], rows_kg[0]) and rows_kg[-1] == ec_add(rows_kg[-2], rows_kg[0])
    dig = FP.table_digits(lib, FP.affine_rows(rows_kg))
    pairs = FP.false_positive_pairs(lib, dig)  # asserts code == kAccMaybeEqual and P != 0, both orders, every sign
    print("false-positive pairs (k_i, k_j):", [(i + 1, j + 1) for i, j in pairs])
    assert len(pairs) >= 4, pairs
    for i, j in pairs:
        assert rows_kg[i][0] != rows_kg[j][0]
        want = ec_add(rows_kg[i], rows_kg[j])
        if i + j + 1 < len(rows_kg):
            assert want == rows_kg[i + j + 1]  # (k_i + k_j) G
        for a, b in ((i, j), (j, i)):
            acc = I52()
            for r in (a, b):
                lib.f30f_acc_madd(acc, I13(*dig[r, :13].tolist()), I13(*dig[r, 13:].tolist()), 0)
            assert affine_of(acc) == want
            check_bounds(acc)
            acc = I52()
            for r in (a, b):
                lib.f30f_acc_madd(acc, I13(*dig[r, :13].tolist()), I13(*dig[r, 13:].tolist()), 1)
            assert affine_of(acc) == (want[0], (-want[1]) % P)
