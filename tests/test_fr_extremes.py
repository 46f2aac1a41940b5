"""CPU: the Fr kernels' accumulation patterns replayed on the host build of the unchanged csrc/fr30.hip.h
(tests/host/fr_reach_host.cpp) under the input families of tests/fr_extremes.py.

(a) every digit, top digit and product column stays inside the contract fr30.hip.h states,
(b) every result equals the Python integer,
(c) the families really fill the bounds: the reach of each pattern is at least 0.9 of the figure measured on the headers of
    the commit that added this test (REACH below, DESIGN.md "Fr magnitudes under test"), and the two figures the sums were
    sized for are asserted outright (256-term sum: 0.85 of kR9SumTopBound; 11-stage NTT chain: 6 r),
(d) teeth: two deliberately weakened patterns (host only, never on a device) leave the stated contract under the
    extremal families and not under 0 and r - 1.

The GPU side (tests/test_fr_extremes_gpu.py) runs the same families through the kernels; the headers are the same code."""
import ctypes
import os
import random
import subprocess

import pytest

import fr_extremes as FE
import ntt_oracle as NO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = FE.R
TOP_R = R / 2.0**240          # the top digit of r
COL = float(1 << 63)
NORM_HARD = (1 << 31) - (1 << 29)  # fr30_norm's own operand limit: past it the carry of a digit overflows 32 bits
U32x8 = ctypes.c_uint32 * 8
REP = ctypes.c_uint64 * 4

# Reach measured with this program on the headers of the commit that added it: the largest |value| in units of r (top
# digit / 0x73ed.a8) and the largest |column| in units of 2^63, over the extremal families of each pattern.
REACH = {
    "mac256": (128.99, 0.296),        # 0.913 of kR9SumTopBound with a canonical start value
    "horner_scan": (1.499, 0.292),
    "horner_cmb": (1.499, 0.520),
    "ntt_chain_11": (6.50, 0.177),
    "ntt_chain_10": (6.00, 0.156),
    "bary_run": (1.99, 0.166),
    "bary_tile": (127.9, 0.156),
    "bary_finish": (63.9, 0.194),
    "fold_first": (7.99, 0.136),
    "fold_second": (1.96, 0.114),
}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fre") / "libfre.so")
    # -fwrapv: a weakened variant may overflow a 32-bit digit sum; the device wraps, and so must this build
    subprocess.run(["g++", "-O2", "-fwrapv", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "host", "fr_reach_host.cpp")],
                   check=True)
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def bounds(lib):
    b = (ctypes.c_int64 * 3)()
    lib.fre_bounds(b)
    assert list(b) == [(1 << 30) + 4, (1 << 29) + 4, 1 << 22]
    return list(b)


def _u32(images):
    b = b"".join(int(v).to_bytes(32, "little") for v in images)
    return (ctypes.c_uint32 * (8 * len(images))).from_buffer_copy(b)


def _mults(ws):
    """plain multipliers -> their blst_fr images, 4 x u64 each"""
    b = b"".join((int(w) % R * FE.R256 % R).to_bytes(32, "little") for w in ws)
    return (ctypes.c_uint64 * (4 * len(ws))).from_buffer_copy(b)


def _val(buf, i=0):
    return int.from_bytes(bytes(buf)[32 * i:32 * i + 32], "little")


class Report:
    def __init__(self, rep, ok):
        self.raw, self.norm, self.top, self.col = [int(x) for x in rep]
        self.ok = ok

    def in_contract(self, bounds):
        return self.raw <= bounds[0] and self.norm <= bounds[1] and self.top < bounds[2] and self.col < (1 << 63)

    def in_hard_limits(self):
        """what the arithmetic itself needs: no 32-bit digit carry and no 64-bit column overflows"""
        return self.raw < NORM_HARD and self.col < (1 << 63)

    def reach(self):
        return self.top / TOP_R, self.col / COL

    def __repr__(self):
        return "raw %.4f x 2^30, norm %.4f x 2^29, top %d (%.3f r), column %.3f x 2^63, %s" % (
            self.raw / 2.0**30, self.norm / 2.0**29, self.top, self.top / TOP_R, self.col / COL, "right" if self.ok else "WRONG")


def run_mac(lib, coeffs, ws, every=1, start=0):
    out, rep = U32x8(), REP()
    lib.fre_mac(_u32([start]), _u32(coeffs), _mults(ws), len(coeffs), every, out, rep)
    return Report(rep, _val(out) == (start + sum(c * w for c, w in zip(coeffs, ws))) % R)


def run_horner(lib, a, z, form, b=None, zl=1):
    n = len(a)
    out, rep = (ctypes.c_uint32 * (8 * (n if form == 0 else 1)))(), REP()
    lib.fre_horner(_u32(a), _u32(b) if b else None, n, _mults([z]), _mults([zl]), form, out, rep)
    h, want = 0, [0] * n
    for i in range(n - 1, -1, -1):
        h = (h * z + a[i] + (b[i] if b else 0)) % R
        want[i] = h
    ok = [_val(out, i) for i in range(n)] == want if form == 0 else _val(out) == want[0] * zl % R
    return Report(rep, ok)


def run_ntt(lib, x, m, inverse=False, last=1):
    n = 1 << m
    w = NO.domain_root(m)
    if inverse:
        w = pow(w, R - 2, R)
    roots = [pow(w, j, R) for j in range(max(n // 2, 1))]
    out, rep = (ctypes.c_uint32 * (8 * n))(), REP()
    lib.fre_ntt(_u32(x), m, _mults(roots), _mults([last]), out, rep)
    want = NO.ntt(x) if not inverse else [v * n % R for v in NO.intt(x)]
    return Report(rep, [_val(out, i) for i in range(n)] == [v * last % R for v in want])


def run_bary(lib, f, ms, factor):
    assert len(f) % 1024 == 0
    out, rep = U32x8(), REP()
    lib.fre_bary(_u32(f), _mults(ms), len(f) // 1024, _mults([factor]), out, rep)
    return Report(rep, _val(out) == factor * sum(a * b for a, b in zip(f, ms)) % R)


def run_fold(lib, values, rhos, fold=16):
    out, rep = U32x8(), REP()
    lib.fre_fold(_u32(values), _mults(rhos), len(values), fold, out, rep)
    return Report(rep, _val(out) == sum(a * b for a, b in zip(values, rhos)) % R)


def _geometric(seed, n):
    """(g^i, g^-i) for a random g: n known multipliers and their inverses without n inversions"""
    g = random.Random(seed).randrange(2, R)
    gi = pow(g, -1, R)
    a, b, x, y = [], [], 1, 1
    for _ in range(n):
        a.append(x)
        b.append(y)
        x, y = x * g % R, y * gi % R
    return a, b


def _check(name, reports, bounds, key=None, top_bound=None):
    """(a) and (b) for every report; (c) for the pattern's reach when key is given"""
    lim = list(bounds)
    if top_bound is not None:
        lim[2] = top_bound
    for label, rp in reports.items():
        print("%-14s %-22s %r" % (name, label, rp))
        assert rp.ok, (name, label, rp)
        assert rp.in_contract(lim), (name, label, rp)
    if key:
        top = max(rp.reach()[0] for rp in reports.values())
        col = max(rp.reach()[1] for rp in reports.values())
        print("%-14s reach %.3f r, column %.3f x 2^63 (measured %r)" % (name, top, col, REACH[key]))
        assert top >= 0.9 * REACH[key][0] and col >= 0.9 * REACH[key][1], (name, top, col, REACH[key])
        return top, col


# ---- the families themselves ----------------------------------------------------------------------------------------


def test_families_are_canonical_and_extremal():
    for v in FE.half_values() + FE.digit_extremal():
        assert 0 < v < R
    assert FE.centred(FE.H_PLUS) == (R - 1) // 2 and FE.centred(FE.H_MINUS) == -(R - 1) // 2
    assert FE.centred(R - 1) == -1  # the smallest non-zero magnitude, not the largest
    for t in FE.TOPS:
        assert FE.balanced_digits(FE.d_plus(t))[:8] == [(1 << 29) - 1] * 8
        assert FE.balanced_digits(FE.d_minus(t))[:8] == [-(1 << 29)] + [-(1 << 29) + 1] * 7
        assert FE.balanced_digits(FE.d_alt(t, 1))[:8] == [-(1 << 29), 1 << 29] * 4
        assert all(abs(d) >= (1 << 29) - 1 for d in FE.balanced_digits(FE.d_alt(t, 0))[1:8])
    for m in (FE.H_PLUS, FE.d_minus(0), FE.d_alt(0x73EC)):
        assert FE.multiplier_for(m) * FE.R270 % R == m
        assert FE.multiplier_image_for(m) == FE.multiplier_for(m) * FE.R256 % R
    ms = [3, 5, R - 2]
    assert [c * m % R for c, m in zip(FE.compensated(ms), ms)] == [FE.H_PLUS] * 3
    assert [FE.ntt_plan(k) for k in (0, 1, 11, 12, 18, 20, 22)] == [[0], [1], [11], [6, 6], [9, 9], [7, 7, 6], [8, 7, 7]]
    x, m = FE.ntt_chain(12)
    assert m == 6 and sorted(x) == [0] + [64 << t for t in range(6)] and x[0] == R - 1


# ---- (a) (b) (c) ----------------------------------------------------------------------------------------------------


def _mac_families():
    gs, gis = _geometric(1, 256)
    fams = {"H+ gamma=1": ([FE.H_PLUS] * 256, [1] * 256, 0), "H- gamma=1": ([FE.H_MINUS] * 256, [1] * 256, 0),
            "H+ gamma=1 from r-1": ([FE.H_PLUS] * 256, [1] * 256, R - 1),
            "H+ compensated": ([FE.H_PLUS * x % R for x in gis], gs, 0),
            "H- compensated": ([FE.H_MINUS * x % R for x in gis], gs, FE.H_MINUS)}
    for i, d in enumerate(FE.digit_extremal()):
        fams["D%d gamma=1" % i] = ([d] * 256, [1] * 256, 0)
        fams["D%d M=D" % i] = ([d] * 256, [FE.multiplier_for(d)] * 256, d)
    for i, h in enumerate(FE.half_values()[2:]):
        fams["H%d gamma=1" % i] = ([h] * 256, [1] * 256, 0)
    return fams


def test_sum_of_256_products(lib, bounds):
    """the fr30_mac loop of k_combine_eval and k_sets_combine"""
    reports = {k: run_mac(lib, c, w, 1, s) for k, (c, w, s) in _mac_families().items()}
    top, _ = _check("mac256", reports, bounds, "mac256")
    assert reports["H+ gamma=1"].top >= 0.85 * bounds[2] and reports["H- gamma=1"].top >= 0.85 * bounds[2]
    assert reports["H+ compensated"].top >= 0.85 * bounds[2]
    # r - 1 is no extreme: every product is -1
    small = run_mac(lib, [R - 1] * 256, [1] * 256)
    assert small.ok and small.top <= 0x73EE and small.raw <= 256


HORNER_N = 300


def _horner_cases():
    rng = random.Random(2)
    zs = {"1": 1, "random": rng.randrange(R)}
    for i, w in enumerate(FE.extremal_multipliers()):
        zs["M%d" % i] = w
    coeffs = {"D+": [FE.d_plus(0)] * HORNER_N, "D-": [FE.d_minus(0)] * HORNER_N,
              "alt": [FE.d_alt(0, i & 1) for i in range(HORNER_N)],
              "D+t": [FE.d_plus(0x73EC)] * HORNER_N, "D-t": [FE.d_minus(0x73EC)] * HORNER_N,
              "altt": [FE.d_alt(0x73EC, i & 1) for i in range(HORNER_N)], "H+": [FE.H_PLUS] * HORNER_N}
    return zs, coeffs


def test_horner_steps(lib, bounds):
    """fr30_mul_add of the quotient scans (form 0) and the raw step of cmb_steps (form 1)"""
    zs, coeffs = _horner_cases()
    for form, key in ((0, "horner_scan"), (1, "horner_cmb")):
        reports = {"z %s, %s" % (zk, ck): run_horner(lib, a, z, form, zl=zs["M3"]) for zk, z in zs.items() for ck, a in coeffs.items()}
        _check(key, reports, bounds, key)


def test_ntt_stages(lib, bounds):
    """the DIT stages of k_ntt_pass; the comment allows 10 r (top digit below 2^20), canonical inputs reach 7 r at most:
    2 r after the product-free first stage and 0.5 r per later stage"""
    reach = {}
    for k in (1, 2, 10, 11, 12, 18, 20):
        reports = {}
        for name, h in (("H+", FE.H_PLUS), ("H-", FE.H_MINUS)):
            small, m = FE.ntt_chain_small(k, h)
            reports["chain %s forward" % name] = run_ntt(lib, small, m)
            reports["chain %s inverse" % name] = run_ntt(lib, small, m, True, pow(1 << k, -1, R))
        reach[k] = _check("ntt k=%d" % k, reports, bounds, {10: "ntt_chain_10", 11: "ntt_chain_11"}.get(k), top_bound=1 << 20)
    assert reach[11][0] >= 6.0
    small, m = FE.ntt_chain_small(11, FE.H_PLUS, partner=R - 1)  # the most a canonical input reaches: 7 r of the comment's 10 r
    full = run_ntt(lib, small, m)
    _check("ntt k=11", {"chain with r-1 as the first partner": full}, bounds, top_bound=1 << 20)
    assert 6.99 <= full.reach()[0] <= 7.01
    vectors = {"H+": [FE.H_PLUS] * 2048, "H+ H-": [FE.H_PLUS, FE.H_MINUS] * 1024,
               "D+ D-": [FE.d_plus(0x73EC), FE.d_minus(0x73EC)] * 1024, "alt": [FE.d_alt(0, 1), FE.d_alt(0x73EC, 0)] * 1024,
               "r-1": [R - 1] * 2048}
    reports = {k: run_ntt(lib, v, 11) for k, v in vectors.items()}
    _check("ntt vectors", reports, bounds, top_bound=1 << 20)
    assert reports["r-1"].reach()[0] < 2.01  # what the suite's worst case reached before


def test_barycentric_sums(lib, bounds):
    """run (4 terms), tile (256 runs) and finish (tiles / 64 per lane, then 64 lanes) of k_bary_partial / k_bary_finish.
    A level is filled when ITS terms are all congruent to H: the sum of 4 H is -2, so one input fills one level."""
    factor = random.Random(3).randrange(R)
    for tiles, level, scale, key in ((1, "run", 1, "bary_run"), (1, "tile", 4, "bary_tile"), (128, "run", 1, None),
                                     (128, "tile", 4, None), (128, "finish", 1024, "bary_finish")):
        ms, mis = _geometric(4 + tiles, 1024 * tiles)
        reports = {}
        for name, h in (("H+", FE.H_PLUS), ("H-", FE.H_MINUS)):
            target = h * pow(scale, -1, R) % R
            reports["%s at the %s level, %d tiles" % (name, level, tiles)] = run_bary(lib, [target * x % R for x in mis], ms, factor)
        _check("bary", reports, bounds, key, top_bound=1 << 26)  # the comment: sums below 2^266
    reports = {"D+ D-": run_bary(lib, [FE.d_plus(0x73EC), FE.d_minus(0x73EC)] * 512, _geometric(9, 1024)[0], factor),
               "r-1": run_bary(lib, [R - 1] * 1024, [1] * 1024, factor)}
    _check("bary", reports, bounds, top_bound=1 << 26)


def test_verifier_fold(lib, bounds):
    """k_vc_fr_sum: 33 rows of one cell id are two full folds of 16 and one more, then a fold of three"""
    rng = random.Random(5)
    rhos = [rng.randrange(1, R) for _ in range(33)]
    ext = (FE.extremal_multipliers() * 6)[:33]
    for scale, key in ((1, "fold_first"), (16, "fold_second")):
        reports = {}
        for name, h in (("H+", FE.H_PLUS), ("H-", FE.H_MINUS)):
            reports[name] = run_fold(lib, FE.compensated(rhos, h * pow(scale, -1, R) % R), rhos)
            reports[name + " extremal weights"] = run_fold(lib, FE.compensated(ext, h * pow(scale, -1, R) % R), ext)
        _check("fold", reports, bounds, key, top_bound=1 << 20)  # the comment: |sum| < 2^260
    _check("fold", {"D+ D-": run_fold(lib, [FE.d_plus(0x73EC), FE.d_minus(0x73EC), FE.d_alt(0x73EC)] * 11, ext)}, bounds,
           top_bound=1 << 20)


# ---- (d) teeth ------------------------------------------------------------------------------------------------------
# The weakened variants: fr30_mac with a carry pass after every second product, and the raw Horner step with a raw sum of
# three.  Both leave the contract fr30.hip.h states (a raw digit past kR9SumRawBound) under the extremal families, and stay
# inside it under 0 and r - 1 -- which is why the suite's former extremes could not tell such an edit from the kernel.
# What the replay also shows: neither variant returns a wrong integer under ANY family.  The stated bounds keep one term
# of slack: the largest raw sum of three is 2^29 + 2 (2^29 - 1) = 3 * 2^29 - 2, just below the 3 * 2^29 at which the carry
# of fr30_norm overflows, and the largest column of a product with a raw sum of three is 0.72 * 2^63.  Random inputs
# therefore pass kR9SumRawBound too (three digits uniform in +-2^29 sum past 2^30 with probability 1/24 per digit): for
# them the test asserts the right integer and the arithmetic's own limits, not the stated contract.


def test_weakened_mac_leaves_the_contract_only_under_the_extremal_families(lib, bounds):
    fams = _mac_families()
    for k in ("H+ gamma=1", "H- gamma=1", "H+ compensated", "H- compensated", "D0 M=D", "D1 M=D", "D6 M=D"):
        c, w, s = fams[k]
        weak, real = run_mac(lib, c, w, 2, s), run_mac(lib, c, w, 1, s)
        print("mac / 2  %-20s %r" % (k, weak))
        assert not weak.in_contract(bounds) or not weak.ok, (k, weak)
        assert real.in_contract(bounds) and real.ok
    gs, _ = _geometric(1, 256)
    for k, (c, w) in {"zero": ([0] * 256, gs), "r-1": ([R - 1] * 256, [1] * 256), "r-1 times r-1": ([R - 1] * 256, [R - 1] * 256)}.items():
        weak = run_mac(lib, c, w, 2)
        assert weak.in_contract(bounds) and weak.ok, (k, weak)
    rng = random.Random(6)
    worst = 0
    for it in range(1000):
        t = rng.choice([2, 3, 16])
        weak = run_mac(lib, [rng.randrange(R) for _ in range(t)], [rng.randrange(R) for _ in range(t)], 2, rng.randrange(R))
        assert weak.ok and weak.in_hard_limits(), (it, weak)
        worst = max(worst, weak.raw)
    print("mac / 2  random: largest raw digit %.4f x 2^30" % (worst / 2.0**30))


def test_weakened_horner_leaves_the_contract_only_under_the_extremal_families(lib, bounds):
    zs, coeffs = _horner_cases()
    for zk in ("random", "M0", "M2", "M3", "M5"):
        for ck in ("D+", "D-", "alt", "D+t", "D-t", "altt"):
            weak = run_horner(lib, coeffs[ck], zs[zk], 1, b=coeffs[ck], zl=zs["M3"])
            print("horner 3 z %-7s %-5s %r" % (zk, ck, weak))
            assert not weak.in_contract(bounds) or not weak.ok, (zk, ck, weak)
            real = run_horner(lib, coeffs[ck], zs[zk], 1, zl=zs["M3"])
            assert real.in_contract(bounds) and real.ok
    for k, a in {"zero": [0] * HORNER_N, "r-1": [R - 1] * HORNER_N}.items():
        weak = run_horner(lib, a, 1, 1, b=a)
        assert weak.in_contract(bounds) and weak.ok, (k, weak)
    rng = random.Random(7)
    for it in range(1000):
        n = rng.choice([1, 2, 8])
        a, b = [rng.randrange(R) for _ in range(n)], [rng.randrange(R) for _ in range(n)]
        weak = run_horner(lib, a, rng.randrange(R), 1, b=b, zl=rng.randrange(R))
        assert weak.ok and weak.in_hard_limits(), (it, weak)
