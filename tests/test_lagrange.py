"""CPU: tests/lagrange_oracle.py against itself and against the coefficient route of tests/ntt_oracle.py, and the arithmetic of
the evaluation-form quotient kernels (csrc/lagrange_kernels.hip) replayed on the host at the magnitudes their bound comments
allow (tests/host/lagrange_reach_host.cpp: a stand-alone program built with g++, nothing is loaded into this process)."""
import os
import random
import subprocess

import pytest

import fr_extremes as FE
import lagrange_oracle as LO
import ntt_oracle as NO

R = NO.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 8, 2048]


def _evals(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R) for _ in range(n)]


def _poly_eval(c, x):
    acc = 0
    for v in reversed(c):
        acc = (acc * x + v) % R
    return acc


def _points(n):
    """z outside the domain, then w^m for m = 0, n - 1, n / 2"""
    w = NO.domain_root(NO.log2_exact(n))
    return [0x1234567 + n] + [pow(w, m, R) for m in sorted({0, n - 1, n // 2})]


@pytest.mark.parametrize("n", SIZES)
def test_lagrange_values_interpolate(n):
    k = NO.log2_exact(n)
    e = _evals(n, n)
    c = NO.intt(e)
    for s in _points(n) + [5]:
        ls = LO.lagrange_at(k, s)
        assert sum(f * l for f, l in zip(e, ls)) % R == _poly_eval(c, s), s
        assert sum(ls) % R == 1  # the basis sums to the constant one
    pts = LO.domain(k)
    for m in sorted({0, n - 1, n // 2}):  # the in-domain limit: 1 at s = w^i, 0 at the other domain points
        assert LO.lagrange_at(k, pts[m]) == [1 if i == m else 0 for i in range(n)]


@pytest.mark.parametrize("n", SIZES)
def test_quotient_values_equal_the_transform_of_the_coefficient_quotient(n):
    e = _evals(n, 100 + n)
    c = NO.intt(e)
    for z in _points(n):
        y = _poly_eval(c, z)
        q, acc = [0] * n, 0
        for i in range(n - 1, 0, -1):  # synthetic division of P - y by X - z, high to low
            acc = (acc * z + c[i]) % R
            q[i - 1] = acc
        assert LO.quotient_evals(e, z, y) == NO.ntt(q), z


def test_bit_reversal_helpers():
    assert [LO.brp(i, 3) for i in range(8)] == [0, 4, 2, 6, 1, 5, 3, 7]
    assert LO.brp(0, 0) == 0
    items = list(range(16))
    assert LO.bit_reverse(LO.bit_reverse(items)) == items and LO.bit_reverse(items)[1] == 8


# ---- the kernels' arithmetic at its bounds -------------------------------------------------------------------------------------
RAW_BOUND = (1 << 30) + 8    # a difference of two carry-normalised values, or a normalised sum plus a product
NORM_BOUND = (1 << 29) + 4   # what fr30_norm, a load and a product leave in digits 0..7 (fr30.hip.h)
TOP_BOUND = 1 << 27          # the finish kernel's sums: below 2100 r (lagrange_kernels.hip, "Bounds")
COLUMN_BOUND = 1 << 63       # a product's column fits the signed 64-bit accumulator


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lagrange") / "lagrange_reach")
    # -fwrapv: a digit sum that overflowed would wrap on the device, and so must it here
    subprocess.run(["g++", "-O2", "-fwrapv", "-o", exe, os.path.join(ROOT, "tests", "host", "lagrange_reach_host.cpp")], check=True)

    def run(tiles, y, elements):
        """elements: (f image, plain w, plain dinv); returns (report, sum f w dinv, sum q w, differs, q of the elements)"""
        img = lambda v: "%064x" % (v % R * FE.R256 % R)
        text = "%d %d %064x\n" % (tiles, len(elements), y) + "".join("%064x %s %s\n" % (f, img(w), img(d)) for f, w, d in elements)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
        rep = [int(v) for v in out[:4]]
        return rep, int(out[4], 16), int(out[5], 16), int(out[6]), [int(v, 16) for v in out[7:]]

    return run


def _check_report(rep):
    assert rep[0] <= RAW_BOUND and rep[1] <= NORM_BOUND and rep[2] < TOP_BOUND and rep[3] < COLUMN_BOUND, rep


def _expected(tiles, y, elements):
    count = tiles * 1024 // len(elements)
    bary = sum(f * w % R * d for f, w, d in elements) * count % R
    qs = [(y - f) * d % R for f, w, d in elements]
    dom = sum(q * w for q, (f, w, d) in zip(qs, elements)) * count % R
    return bary, dom, qs


@pytest.mark.parametrize("tiles", [1, 4096])
def test_replay_extremal_values_and_multipliers(replay, tiles):
    """every pairing of an extremal value with an extremal multiplier, f_i - y at both signs (y = 0, r - 1 and a half value)"""
    values = FE.half_values() + FE.digit_extremal() + [0, 1, R - 1]
    mults = FE.extremal_multipliers()
    for y in (0, R - 1, FE.H_PLUS, FE.d_minus(0x73EC)):
        elements = [(values[(3 * i + j) % len(values)], mults[i % len(mults)], mults[(i + j) % len(mults)])
                    for i, j in ((i, i // len(mults)) for i in range(32))]
        rep, bary, dom, differs, qs = replay(tiles, y, elements)
        _check_report(rep)
        want = _expected(tiles, y, elements)
        assert (bary, dom, qs) == want and differs == 1, y


@pytest.mark.parametrize("h", [FE.H_PLUS, FE.H_MINUS])
@pytest.mark.parametrize("level", [1, 4, 1024])
def test_replay_sums_of_one_sign(replay, h, level):
    """Compensated terms: `level` equal terms add up to a half value, so that the sums of one level all have one sign and that
    level reaches what its comment allows -- level 1: every product is +-r/2 and a run of 4 reaches 2 r; level 4: every run
    comes back from its reduction as +-r/2 and the tile's tree reaches 128 r; level 1024: every tile record is +-r/2 and the
    finish kernel's sum over 4096 tiles reaches 2048 r.  (A reduction returns the centred residue of the true sum, so one input
    cannot hold every level at its extreme at once.)  The constant input also leaves `differs` unset."""
    w, d = FE.extremal_multipliers()[2], FE.extremal_multipliers()[4]
    t = h * pow(level, -1, R) % R
    reach = {1: 2, 4: 128, 1024: 2048}[level]
    f = t * pow(w * d, -1, R) % R                 # f w dinv = t: the barycentric sum
    rep, bary, dom, differs, qs = replay(4096, 0, [(f, w, d)])
    _check_report(rep)
    assert (bary, dom, qs) == _expected(4096, 0, [(f, w, d)]) and differs == 0
    assert rep[2] > (reach - 1) * 0x73ED, rep     # the sum did grow that far (r = 0x73ed... x 2^240)
    y = (f + t * pow(w * d, -1, R)) % R           # (y - f) dinv w = t: the in-domain sum
    rep, bary, dom, differs, qs = replay(4096, y, [(f, w, d)])
    _check_report(rep)
    assert (bary, dom, qs) == _expected(4096, y, [(f, w, d)])
    assert rep[2] > (reach - 1) * 0x73ED, rep
