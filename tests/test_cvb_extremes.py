"""CPU: the arithmetic of the batch verifier's Fr kernels (csrc/circuit_verify_kernels.hip) replayed on the
host build of the unchanged csrc/fr30.hip.h (tests/host/cvb_reach_host.cpp: a stand-alone program built with g++, nothing is loaded
into this process) under the input families of tests/cvb_extremes.py.

(a) every digit, top digit and product column stays inside the contract fr30.hip.h and the unit's "Bounds" paragraph state, and every
    operand of fr30_to_limbs lies inside (-r, 2r);
(b) every result -- PI(zeta) and the hit, the four values of k_cvb_lin, every lane of k_cvb_scalars, every split -- equals the Python
    integer, zero verdicts included;
(c) the families fill the bounds: at least 0.9 of the reach measured on the headers of the commit that added this test (REACH below,
    DESIGN.md section 4.2c), and at least 3 times what {0, 1, r - 1, random} reach on the g0 chain and on the 64 lanes' total;
(d) teeth: two weakened variants (host only, never on a device) -- see test_the_weakened_variants.

The split targets and the ladder's choice of operand are checked in the exponent (cvb_extremes.ladder).  The GPU side
(tests/test_cvb_extremes_gpu.py) runs the same families through the kernels."""
import os
import random
import re
import subprocess

import pytest

import cvb_extremes as CE
import fr_extremes as FE
import ntt_oracle as NO

R = CE.R
ROOT = CE.ROOT
TOP_R = R / 2.0**240  # the top digit of r
SUMS = ("z_w", "acc", "total", "zn_1", "a_gamma", "factor", "sc_z", "konst", "g0", "g01")

# Reach measured with this program on the headers of the commit that added it, over the extremal families: the largest |value| that
# leaves the carry pass of a sum in units of r (top digit / 0x73ed.a8), and the largest |column| in units of 2^63.
REACH = {
    "factor": 1.499,   # abar_j + gamma + beta k_j zeta, three terms of one sign (compensated "lin")
    "konst": 1.497,    # PI - alpha B (abar + gamma) - alpha^2 L_0, three terms of one sign (compensated "g0")
    "g0": 7.99,        # t = 7: the constant and 2t - 1 = 13 subtractions of one sign (compensated "g0")
    "g01": 8.49,       # ... and g1: 2t + 3 = 17 terms
    "total": 31.98,    # 64 lanes at r / 2 (compensated public inputs)
    "acc": 1.0,        # PI's running sum before its reducing product: two terms
    "column": 0.26,    # two normalised operands, no raw sum of two: 9 x 2^58 = 0.28 at most
}
# ... and what {0, 1, r - 1, random} reach there (the suite before this test): printed by test_the_families_reach_the_bounds
RATIO = 3.0


def _top(c):
    """|digit 8| of a value below c r in magnitude with balanced lower digits: c r / 2^240 rounded up, plus the half digit"""
    return (int(c * 10000) * 0x73EE + 9999) // 10000 + 1


def top_bounds(t):
    """the unit's Bounds paragraph, sum by sum: terms of magnitude <= 0.5001 r each"""
    p = 0.5001
    return {"z_w": _top(2 * p), "acc": _top(0.51 + p), "total": _top(64 * 0.51), "zn_1": _top(2 * p), "a_gamma": _top(2 * p),
            "factor": _top(3 * p), "sc_z": _top(2 * p), "konst": _top(3 * p), "g0": _top((2 * t + 2) * p), "g01": _top((2 * t + 3) * p)}


# A product is |p| <= 0.5001 r + |a| |b| / 2^270.  The replay takes |a| |b| / 2^270 off every product, so each is held to the 0.5001 r
# that is its own (PRODUCT_OWN); the top digit of any product stays under the one that takes the lanes' total besides
# (|a| <= 64 x 0.51 r, |b| <= 0.5001 r, r / 2^270 < 2^-15).
PRODUCT_OWN = 0.5001
PRODUCT_TOP = _top(0.5007)


class Run:
    def __init__(self, out):
        lines = out.strip().split("\n")
        self.bounds = [int(x) for x in lines[0].split()]
        rep = [int(x) for x in lines[1].split()]
        k = len(SUMS)
        assert len(rep) == 2 * k + 9
        self.raw, self.top = dict(zip(SUMS, rep[:k])), dict(zip(SUMS, rep[k:2 * k]))
        self.norm, self.prod_top, self.column = rep[2 * k:2 * k + 3]
        self.lo, self.hi, self.outside = rep[2 * k + 3] / 2.0**20, rep[2 * k + 4] / 2.0**20, rep[2 * k + 5]
        self.at_minus_r, self.at_plus_r, self.product_own = rep[2 * k + 6], rep[2 * k + 7], rep[2 * k + 8] / 2.0**20
        self.records, cur = [], None
        for ln in lines[2:]:
            f = ln.split()
            if f[0] == "pi":
                cur = {"pi": int(f[1], 16), "hit": int(f[2]), "lanes": [], "splits": []}
                self.records.append(cur)
            elif f[0] == "lin":
                cur["lin"] = [int(x, 16) for x in f[1:]]
            else:
                cur["lanes"].append((f[0], int(f[1], 16)))
                if f[0] == "s":
                    cur["splits"].append((int(f[1], 16), int(f[2], 16), int(f[3], 16)))

    def reach(self, name):
        return self.column / 2.0**63 if name == "column" else self.top[name] / TOP_R

    def in_contract(self, t):
        tb = top_bounds(t)
        return (all(self.raw[s] <= self.bounds[0] for s in SUMS) and all(self.top[s] <= tb[s] for s in SUMS) and
                self.norm <= self.bounds[1] and self.prod_top <= PRODUCT_TOP and self.product_own <= PRODUCT_OWN and
                self.column < (1 << 63) and self.outside == 0)

    def __repr__(self):
        return ("raw %s\n  top(r) %s\n  norm %d product top %.4f r, its own part %.6f r, column %.3f x 2^63, fr30_to_limbs in "
                "[%.4f r, %.4f r], %d outside, %d at -r, %d at r" % (
                    {s: "%.4f" % (v / 2.0**30) for s, v in self.raw.items()}, {s: "%.3f" % (v / TOP_R) for s, v in self.top.items()},
                    self.norm, self.prod_top / TOP_R, self.product_own, self.column / 2.0**63, self.lo, self.hi, self.outside,
                    self.at_minus_r, self.at_plus_r))


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cvb") / "cvb_reach")
    # -fwrapv: a digit sum that overflowed would wrap on the device, and so must it here
    subprocess.run(["g++", "-O2", "-fwrapv", "-o", exe, os.path.join(ROOT, "tests", "host", "cvb_reach_host.cpp")], check=True)

    def run(shape, consts, records, variant=0):
        """shape: (t, lg_n, e, exps); consts: plain (w, w1, invn, w64, shifts); records: (five, rho, evals, public), plain values"""
        t, lg_n, e, exps = shape
        img = lambda v: "%064x" % (v % R * FE.R256 % R)  # noqa: E731
        n_public = len(records[0][3])
        assert all(len(r[3]) == n_public and len(r[2]) == 2 * t for r in records)
        text = "%d %d %d %d %d %d %d\n" % (variant, t, lg_n, e, len(exps or []), n_public, len(records))
        text += " ".join(str(p) for row in exps or [] for p in row) + "\n"
        text += " ".join(img(v) for v in list(consts[:4]) + list(consts[4])) + "\n"
        for five, rho, evals, public in records:
            text += " ".join(img(v) for v in list(five) + [rho] + list(evals) + list(public)) + "\n"
        return Run(subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout)

    return run


def wrong(shape, consts, records, run):
    """the records whose replayed results differ from the Python integers"""
    t, lg_n, e, exps = shape
    bad = []
    for k, ((five, rho, evals, public), got) in enumerate(zip(records, run.records)):
        pi, hit, lin, lanes = CE.model_lanes(t, lg_n, e, exps, consts, five, rho, evals, public)
        if (got["pi"], got["hit"], got["lin"], got["lanes"]) != (pi, hit, lin, lanes):
            bad.append(k)
        for v, k1, k2 in got["splits"]:
            if (k1, k2) != CE.split(v):
                bad.append(k)
    assert len(run.records) == len(records)
    return bad


# (t, lg_n, e, exponents)
PLAIN3, PLAIN7, CUSTOM, N256 = (3, 3, 4, None), (7, 6, 8, None), (4, 3, 8, CE.CUSTOM_EXPS), (3, 8, 4, None)


def real_consts(shape):
    t, lg_n = shape[0], shape[1]
    w = NO.domain_root(lg_n)
    return (w, (1 + w) % R, pow(1 << lg_n, -1, R), pow(w, 64, R), CE.GO.shifts(t))


def extremal_consts(shape):
    """w, 1 + w, 1 / n and w^64 in the multiplier forms H+, D-, H-, D+ with the top digit just below r's; the shifts stay"""
    m = FE.multiplier_for
    return (m(FE.H_PLUS), m(FE.d_minus(0)), m(FE.H_MINUS), m(FE.d_plus(0x73EC)), CE.GO.shifts(shape[0]))


def cycled_records(values, t, count, n_public):
    out = []
    for k in range(count):
        five, evals, rho, public = CE.cycled(values, t, k, n_public)
        out.append((five, rho, evals, public))
    return out


def compensated_records(shape, consts, h, n_public):
    """the "lin" and "g0" families for every column, and compensated public inputs (n_public of them, one round) under each"""
    t = shape[0]
    w, _, _, w64, ks = consts
    wi = [pow(w, i % 64, R) * pow(w64, i // 64, R) % R for i in range(n_public)]
    values = CE.pool()
    out = []
    for k in range(2 * t):
        five, evals = CE.compensated("lin" if k < t else "g0", ks, k, h)
        if k < t:
            public = CE.compensated_public(five[3], wi, h)
        else:  # (with the replay's free constants "n" is what makes its (zeta^n - 1) invn (zeta - 1)^-1 the factor of row 0)
            public = CE.public_for(-FE.multiplier_for(h) % R, 1 << shape[1], five[3], n_public)
        out.append((five, CE.cycle(values, k, 0), evals, public))
    return out


def two_ends():
    """(consts, records): w^65 = w w64 in multiplier form just above r/2 from a product with a large a b / 2^270 (w near r/2, w64
    chosen for it), and 200 values of zeta just below it whose own product has a small one -- the pair found by search, fixed here"""
    m = FE.multiplier_for
    a = 0x37bce2f01782fe77caa26aabebbd1b7608c4ee29982a47ee2e349f9f4b91388c
    y = 0x3fc6558070f6a2b712cf3e0584d7deccf4dcdeab5e8b57655a3c7bbce896
    w = m(a)
    consts = (w, 1, 1, m((R + 1) // 2 + y) * pow(w, -1, R) % R, CE.GO.shifts(3))
    rnd = random.Random(32)
    records = [((3, 5, 7, m((R + 1) // 2 + y - rnd.randrange(1, y)), 11), 1, [1, 2, 3, 4, 5, 6], [9] * 66) for _ in range(200)]
    return consts, records


# multiplier forms (r + 1) / 2 + x of one residue that zeta and w^65 = w w64 (two_ends' w) bring back as DIFFERENT representatives,
# found by search: zeta the lower and w^65 the upper one (the difference is -r), and the other way round (+r)
SAME_RESIDUE_MINUS_R = (0x235e6572a110f4d8ec61d2f59cce6edc60bc6df5fc859489fb5049d63aa6,
                        0x19881e03a09073eae43574e06261fa652ba2e846e76e4d8b81cce1403c7a)
SAME_RESIDUE_PLUS_R = (0x2fae182156fa4ae66e71083a55371687a15d67d05bdd0ec8646a490c81c0,
                       0x2bd2917cea26eadc52404a6dd8fcab32ac2eeb8767b94c72960289d4aaa3)


def same_residue(x):
    """(consts, records): zeta = w^65 exactly, both (r + 1) / 2 + x in multiplier form; one record, the hit is row 65"""
    m = FE.multiplier_for
    w = two_ends()[0][0]
    zeta = m((R + 1) // 2 + x)
    return (w, 1, 1, zeta * pow(w, -1, R) % R, CE.GO.shifts(3)), [((3, 5, 7, zeta, 11), 1, [1, 2, 3, 4, 5, 6], [9] * 66)]


# ---- the split and the ladder -------------------------------------------------------------------------------------------------
def test_the_replays_split_is_the_units_loop_and_the_targets_split_as_stated():
    def loop(path):
        with open(path) as f:
            text = f.read()
        body = text[text.index("for (int bit = 0; bit < 256; bit++) {"):]
        body = body[:body.index("g.k1[0] = r0;" if "g.k1[0] = r0;" in body else "k1[0] = r0;")]
        return re.sub(r"\s+", " ", body.replace("Glv g;", "")).strip()

    assert loop(CE.UNIT) == loop(os.path.join(ROOT, "tests", "host", "cvb_reach_host.cpp"))
    for k in CE.SPLIT_TARGETS:
        k1, k2 = CE.split(k)
        assert k1 + k2 * CE.LAMBDA == k and k1 < CE.LAMBDA and k2 < 1 << 128 and k1 < 1 << 128
    parts = {k: CE.split(k) for k in CE.SPLIT_TARGETS}
    assert parts[R - 1] == (0, CE.LAMBDA + 1) and parts[CE.LAMBDA] == (0, 1) and parts[0] == (0, 0)
    assert any(k1 == 0 and k2 for k1, k2 in parts.values()) and any(k2 == 0 and k1 for k1, k2 in parts.values())
    assert any(k1 >> 127 for k1, _ in parts.values()) and any(k2 >> 127 for _, k2 in parts.values())


def test_the_targets_reach_every_operand_of_the_ladder_first_and_later():
    """g1_mul_glv in the exponent: the targets take each of the three operands both into infinity (the first addition) and into a
    point, and a ladder whose sel == 2 operand is wrong fails on them"""
    used, caught = set(), []
    for k in CE.SPLIT_TARGETS:
        k1, k2 = CE.split(k)
        for p in (1, 0x1234567, R - 5):
            got, u = CE.ladder(k1, k2, p)
            assert got == k * p % R
            used |= u
            if CE.ladder(k1, k2, p, flip=True)[0] != got:
                caught.append(k)
    assert used == {(sel, when) for sel in (1, 2, 3) for when in ("first", "later")}
    assert {R - 1, CE.LAMBDA, CE.LAMBDA * CE.LAMBDA} <= set(caught)  # k1 = 0: only the sel == 2 operand is ever added


def test_the_model_of_the_lanes_sums_to_the_oracles_three_scalars(oracle):
    """cvb_extremes.model_lanes (what the replay is held to) against circuit_verify_batch_oracle: the lanes' scalars times the
    scalars of their points add up to p0, p1, p2"""
    for which in ("n8", "custom", "t7"):
        st = CE.statement(oracle, which)
        lg_n = NO.log2_exact(st.n)
        consts = (st.w, (1 + st.w) % R, pow(st.n, -1, R), pow(st.w, 64, R), st.ks)
        for k in (0, 3, 11):
            five, evals, rho, public = CE.cycled(CE.pool(), st.t, k, min(5, st.n))
            if k == 3:
                five = five[:3] + (pow(st.w, 2, R),) + five[4:]
            m = st.member(evals, public, st.stock[k % 3])
            want = CE.VB.combine(st.n, [st.contribution(m, five)], [rho])
            _, _, _, lanes = CE.model_lanes(st.t, lg_n, st.e, st.exps, consts, five, rho, evals, public)
            s = [v for _, v in lanes]
            t, e, nk = st.t, st.e, 2 * st.t + 3 + st.g
            own = m.wire_s + [m.z_s] + m.t_s
            D = sum(a * b for a, b in zip(s[:t + e], own)) % R
            E, F = s[t + e] * m.z_s % R, rho * m.w % R
            s2, rows = s[t + e + 1:t + e + 5], s[t + e + 5:]
            key = st.key_s + [1]
            p0 = (s2[0] * D + s2[1] * E + s2[2] * F + sum(a * b for a, b in zip(rows[:nk], key))) % R
            p1 = (D + E + s2[3] * F + sum(a * b for a, b in zip(rows[nk:], key))) % R
            assert (p0, p1, -F % R) == want, (which, k)


# ---- the kernels' arithmetic at its bounds ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("consts_of", [real_consts, extremal_consts], ids=["real", "extremal"])
@pytest.mark.parametrize("shape", [PLAIN3, PLAIN7, CUSTOM], ids=["t3", "t7", "custom"])
def test_replay_contract_and_results_under_the_extremal_families(replay, shape, consts_of):
    t = shape[0]
    consts = consts_of(shape)
    values = CE.pool()
    sets = {"pool": cycled_records(values, t, len(values), 5),
            "pool, no public inputs": cycled_records(values, t, 8, 0),
            "pool, 129 public inputs": cycled_records(values, t, 6, 129),
            "compensated +": compensated_records(shape, consts, CE.HP, 64),
            "compensated -": compensated_records(shape, consts, CE.HM, 64)}
    for name, records in sets.items():
        run = replay(shape, consts, records)
        print("%s\n  %r" % (name, run))
        assert run.bounds == [(1 << 30) + 4, (1 << 29) + 4]
        assert run.in_contract(t), (name, run)
        assert wrong(shape, consts, records, run) == [], name


@pytest.mark.parametrize("consts_of", [real_consts, extremal_consts], ids=["real", "extremal"])
def test_replay_zero_verdicts_on_redundant_forms(replay, consts_of):
    """zeta = 1 and zeta = w^i with zeta's multiplier form near +-r/2, in round 0, in a later round and in the last, partly dead one; past
    the public rows there is no hit.  (With the extremal constants w is H+ in multiplier form: zeta = w is r/2 itself.)"""
    shape = N256
    consts = consts_of(shape)
    w, _, _, w64, _ = consts
    values = CE.pool()
    wi = lambda i: pow(w, i % 64, R) * pow(w64, i // 64, R) % R  # noqa: E731
    records, hits = [], []
    zetas = [wi(i) for i in (0, 1, 63, 64, 100, 128, 129, 200)] + [1, FE.multiplier_for(FE.H_PLUS), FE.multiplier_for(FE.H_MINUS), 0]
    for k, x in enumerate(zetas):
        five, evals, rho, public = CE.cycled(values, 3, k, 129)
        records.append((five[:3] + (x,) + five[4:], rho, evals, public))
        hits.append(next((i for i in range(129) if wi(i) == x), -1))
    assert hits[:8] == [0, 1, 63, 64, 100, 128, -1, -1]
    run = replay(shape, consts, records)
    print(run)
    assert [r["hit"] for r in run.records] == hits
    assert run.in_contract(3) and wrong(shape, consts, records, run) == []


def test_the_families_reach_the_bounds(replay):
    """(c): the reach per pattern, and how far beyond {0, 1, r - 1, random} the families go"""
    shape, consts = PLAIN7, real_consts(PLAIN7)
    best, plain = {}, {}
    for h in (CE.HP, CE.HM):
        run = replay(shape, consts, compensated_records(shape, consts, h, 64))
        for name in REACH:
            best[name] = max(best.get(name, 0), run.reach(name))
    for n_public in (64, 129):
        run = replay(shape, consts, cycled_records(CE.pool(), 7, len(CE.pool()), n_public))
        for name in REACH:
            best[name] = max(best[name], run.reach(name))
    for seed in range(4):
        run = replay(shape, consts, cycled_records(CE.plain_pool(seed), 7, 24, 64))
        assert run.in_contract(7)
        for name in REACH:
            plain[name] = max(plain.get(name, 0), run.reach(name))
    for name in REACH:
        print("%-8s reach %.3f (measured %.3f), {0, 1, r - 1, random} reach %.3f: x %.1f" % (
            name, best[name], REACH[name], plain[name], best[name] / plain[name]))
        assert best[name] >= 0.9 * REACH[name], (name, best[name])
    for name in ("g0", "total"):
        assert best[name] >= RATIO * plain[name], (name, best[name], plain[name])


def test_the_weakened_variants(replay):
    """(d), host only.  Variant 1 makes the zero tests on the unreduced difference z - w^i; variant 2 hands fr30_to_limbs the raw sum
    g0 + g1 without the reducing product.  Under the extremal families each gives a wrong result or an operand of fr30_to_limbs
    outside (-r, 2r); under 0 and r - 1 neither does.  Variant 1 leaves the interval (at -r itself for zero, below -r for non-zero
    differences) and returns no wrong verdict on these inputs, which the test asserts: fr30_to_limbs adds r to any negative operand"""
    shape, consts = PLAIN7, real_consts(PLAIN7)
    t = 7
    small = cycled_records([0, R - 1], t, 8, 5)
    # variant 2: the line of G1's term of P1 holds the residue of the multiplier form of g0 + g1, without rho
    def v2_wrong(records, run):
        bad = 0
        for (five, rho, evals, public), got in zip(records, run.records):
            _, _, lin, _ = CE.model_lanes(t, shape[1], shape[2], None, consts, five, 1, evals, public)
            v = five[4]
            g = (lin[3] - sum(pow(v, i, R) * evals[i - 1] for i in range(1, 2 * t + 1))) % R
            bad += got["lanes"][-1] != ("r", g * FE.R270 % R)
        return bad

    run = replay(shape, consts, small, variant=2)
    assert run.outside == 0 and v2_wrong(small, run) == 0
    comp = compensated_records(shape, consts, CE.HP, 5) + compensated_records(shape, consts, CE.HM, 5)
    run = replay(shape, consts, comp, variant=2)
    print("variant 2: fr30_to_limbs in [%.3f r, %.3f r], %d outside, %d wrong" % (run.lo, run.hi, run.outside, v2_wrong(comp, run)))
    assert run.outside > 0 and v2_wrong(comp, run) > 0
    # variant 1.  A product returns a value in (-r/2 + d, r/2 + d) with d = a b / 2^270, anywhere in [0, r / 2^15) by its operands,
    # so a residue next to r/2 has two representatives.  (i) zeta = w^65 exactly, zeta brought back as the lower one and w^65 as the
    # upper one: the unreduced difference is -r for ZERO, outside (-r, 2r); the other way round it is +r
    for x in SAME_RESIDUE_MINUS_R + SAME_RESIDUE_PLUS_R:
        consts, one = same_residue(x)
        run0 = replay(N256, consts, one)
        assert run0.in_contract(3) and run0.at_minus_r == run0.at_plus_r == 0 and run0.records[0]["hit"] == 65
        assert wrong(N256, consts, one, run0) == []
        run = replay(N256, consts, one, variant=1)
        print("variant 1, zeta = w^65: %d at -r, %d at r, %d outside, hit %d" % (run.at_minus_r, run.at_plus_r, run.outside,
                                                                              run.records[0]["hit"]))
        if x in SAME_RESIDUE_MINUS_R:
            assert (run.at_minus_r, run.at_plus_r, run.outside) == (1, 0, 1)
        else:
            assert (run.at_minus_r, run.at_plus_r, run.outside) == (0, 1, 0)
        # the verdict survives: fr30_to_limbs adds r to any negative operand, so -r comes back as 0 although its contract excludes it
        assert run.records[0]["hit"] == 65 and wrong(N256, consts, one, run) == []
    # (ii) zeta = r/2 + x as -r/2 + x and w^65 = r/2 + y, x < y: a difference below -r that is NOT zero
    consts, near = two_ends()
    run0 = replay(N256, consts, near)
    assert run0.outside == 0 and run0.in_contract(3) and wrong(N256, consts, near, run0) == []
    run = replay(N256, consts, near, variant=1)
    print("variant 1: fr30_to_limbs in [%.6f r, %.6f r], %d outside" % (run.lo, run.hi, run.outside))
    assert run.outside > 0 and run.at_minus_r == 0
    assert wrong(N256, consts, near, run) == []  # limbs that are no residue, but not zero either: the verdicts stand
    small3 = cycled_records([0, R - 1], 3, 8, 5)
    run = replay(PLAIN3, real_consts(PLAIN3), small3, variant=1)
    assert run.outside == 0 and wrong(PLAIN3, real_consts(PLAIN3), small3, run) == []
