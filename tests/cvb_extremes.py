"""Inputs for the batch verifier's Fr kernels and GLV ladders at their edges (csrc/circuit_verify_kernels.hip, DESIGN.md sections 4.2c
and 4.29), and a synthetic statement that needs no prover.  Pure Python integers.

The kernels slice blst_fr IMAGES (x 2^256 mod r) and compute in the multiplier form x 2^270, centred: the magnitude of a value there is
|centred(x 2^270)|, whatever x is.  So the families of tests/fr_extremes.py enter in three ways (pool):
  * as images: x = I 2^-256 for a half value or a digit-extremal integer I -- the digits fr30_from_limbs makes are extremal;
  * as multipliers: x = FE.multiplier_for(M) -- the value the kernels compute with is M, at +-r/2 or with extremal digits;
  * as they are (H+, H-, 0, 1, 2, r - 1).

Compensated inputs (compensated): with h = multiplier_for(H), every term of a chained raw sum is congruent to H with ONE sign:
  * "lin": abar_j = gamma = h, sbar_j = h / beta and beta k_j zeta = h for ONE column j (the shifts differ, so one zeta serves one column;
    the column moves with the proof's index): the three-term sums abar_j + gamma + beta k_j zeta and abar_j + gamma + beta sbar_j of
    k_cvb_lin;
  * "g0": y_i = h / v^i for the 2t - 1 evaluations of the g0 chain and z(zeta w) = h / v^(2t), so that g0 = const - sum v^i y_i moves
    r / 2 the same way 2t - 1 times and g1 once more (k_cvb_scalars); alpha is chosen so that alpha B (abar_(t-1) + gamma) = h and the
    public inputs so that PI(zeta) = -h (public_for): two of the constant's three terms go the same way (the third, alpha^2 L_0, would
    need a square root and keeps the sign it has).
HP and HM (just inside +-r/2, see below) give the two signs; the constant in front has the sign it has, so one of the two accumulates on it.

Split targets: r = lambda^2 + lambda + 1, so r - 1 = (lambda + 1) lambda splits as (0, lambda + 1) -- k1 zero, k2 of 128 bits -- and
r - 2 as (lambda - 1, lambda); lambda itself as (0, 1): the ladder starts at bit 0 and adds into infinity.

The synthetic statement: key commitments [c_j]G and proof points [c]G with c known, evaluations and public inputs free.  Validity is
not needed: kzg_circuit_verify_proofs_lincomb_challenges returns P0, P1, P2 for any decodable batch, and
circuit_verify_batch_oracle.contribution computes the same from the scalars."""
import os
import random
import re
import types

import circuit_verify_batch_oracle as VB
import fr_extremes as FE
import grand_product_oracle as GO
import ntt_oracle as NO
import transcript_oracle as TR
import trapdoor_oracle as TO

R = FE.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = os.path.join(ROOT, "kzg_poly_commit_exploration_amd", "csrc", "circuit_verify_kernels.hip")
INV256 = pow(FE.R256, -1, R)
# A product returns x 2^270 + m r with |x 2^270 - centred| up to r / 2^15 (its |a b| / 2^270), so a residue within that of r / 2 comes
# back with either sign, by the operands.  The compensated families use r / 2 - r / 2^12: one representative, 0.4998 r.
HP = FE.H_PLUS - (R >> 12)
HM = FE.H_MINUS + (R >> 12)


def _lambda():
    with open(UNIT) as f:
        m = re.search(r"kLambdaHi = (0x[0-9a-f]+)ULL, kLambdaLo = (0x[0-9a-f]+)ULL", f.read())
    return int(m.group(1), 16) << 64 | int(m.group(2), 16)


LAMBDA = _lambda()
assert R == LAMBDA * LAMBDA + LAMBDA + 1
SPLIT_TARGETS = [0, 1, 2, (1 << 64) - 1, 1 << 64, 1 << 127, (1 << 128) - 1, 1 << 128, LAMBDA - 1, LAMBDA, LAMBDA + 1, 2 * LAMBDA - 1,
                 (1 << 127) * LAMBDA, LAMBDA * LAMBDA, R - 2, R - 1]
assert all(0 <= k < R for k in SPLIT_TARGETS)


def split(k):
    """(k1, k2) of the canonical scalar k: k = k1 + k2 lambda, k1 < lambda"""
    k2, k1 = divmod(k, LAMBDA)
    return k1, k2


assert split(R - 1) == (0, LAMBDA + 1) and split(R - 2) == (LAMBDA - 1, LAMBDA) and split(LAMBDA) == (0, 1)


def ladder(k1, k2, p, flip=False):
    """g1_mul_glv in the exponent (the point [p]G as the scalar p, phi as the product with lambda): the joint double-and-add with the
    kernel's choice of operand, and the operands each step took.  flip: the sel == 2 operand replaced by p (a WRONG ladder, for the test
    of the targets' teeth).  This is a model written beside the kernel: nothing holds it to g1_mul_glv's text, so its test shows what
    the TARGETS exercise, not that the kernel selects rightly -- that is the GPU test's comparison of the points"""
    acc, used = 0, set()
    bits = max(k1.bit_length(), k2.bit_length())
    both = p * (1 + LAMBDA) % R
    for bit in range(bits - 1, -1, -1):
        acc = 2 * acc % R
        sel = (k1 >> bit & 1) | (k2 >> bit & 1) << 1
        if sel:
            used.add((sel, "first" if acc == 0 else "later"))
            acc = (acc + (p if sel == 1 else ((p if flip else p * LAMBDA) if sel == 2 else both))) % R
    return acc, used


def pool():
    """plain values whose image or whose multiplier form is a half value or digit-extremal, and the small ones"""
    out = [v * INV256 % R for v in FE.half_values() + FE.digit_extremal()]
    out += FE.extremal_multipliers() + [FE.multiplier_for(FE.H_PLUS - 1), FE.multiplier_for(FE.H_MINUS + 1)]
    out += [FE.H_PLUS, FE.H_MINUS, 0, 1, 2, R - 1]
    return out


def plain_pool(seed, count=24):
    """what the suite had before: 0, 1, r - 1 and random values"""
    rnd = random.Random(seed)
    return [0, 1, R - 1] + [rnd.randrange(R) for _ in range(count - 3)]


def cycle(values, k, slot, step=7):
    """value `slot` of proof k: every proof starts at another phase"""
    return values[(step * k + 5 * slot + k // len(values)) % len(values)]


def cycled(values, t, k, n_public=0):
    """(five, evals, rho, public) of proof k, everything from `values`"""
    five = tuple(cycle(values, k, s) for s in range(5))
    evals = [cycle(values, k, 5 + s) for s in range(2 * t)]
    public = [cycle(values, k, 6 + 2 * t + i, 11) for i in range(n_public)]
    return five, evals, cycle(values, k, 5 + 2 * t), public


def compensated(kind, ks, k, h_value=HP, seed=0):
    """(five, evals) of proof k under the compensated family `kind` ("lin" or "g0", see above); the free challenges are random"""
    t = len(ks)
    rnd = random.Random(1000 * seed + k)
    full = lambda: rnd.randrange(1, R)  # noqa: E731
    h = FE.multiplier_for(h_value)
    beta, gamma, alpha, zeta, v = full(), full(), full(), full(), full()
    if kind == "lin":
        gamma = h
        zeta = h * pow(beta * ks[k % t] % R, -1, R) % R
        evals = [h] * t + [h * pow(beta, -1, R) % R] * (t - 1) + [full()]
    else:
        assert kind == "g0"
        vi = pow(v, -1, R)
        evals = [h * pow(vi, i, R) % R for i in range(1, 2 * t + 1)]
        B = evals[2 * t - 1]  # ... and alpha B (abar_(t-1) + gamma) = h: the constant's second term goes the chain's way
        for j in range(t - 1):
            B = B * (evals[j] + gamma + beta * evals[t + j]) % R
        alpha = h * pow(B * (evals[t - 1] + gamma) % R, -1, R) % R
    return (beta, gamma, alpha, zeta, v), evals


def public_for(target, n, zeta, n_public):
    """public inputs (row 0 alone is not zero) with PI(zeta) = target, zeta outside the domain: the constant's first term"""
    p0 = target * n % R * (zeta - 1) % R * pow(pow(zeta, n, R) - 1, -1, R) % R
    return [p0] + [0] * (n_public - 1)


def compensated_public(zeta, wi, h_value=HP):
    """public inputs with PI_i w^i / (zeta - w^i) = h for the given powers wi (zeta is none of them): every lane of k_cvb_public ends
    its first round with a sum congruent to H, and the 64 lanes' total is 64 terms of one sign"""
    h = FE.multiplier_for(h_value)
    return [h * (zeta - x) % R * pow(x, -1, R) % R for x in wi]


# (n, t, log_ext, exponents): the smallest shapes at which each path exists
CUSTOM_EXPS = ((7, 0, 0, 0), (0, 0, 0, 7), (1, 2, 3, 1), (0, 7, 0, 0), (2, 2, 2, 1), (0, 0, 7, 0), (3, 1, 0, 3), (1, 1, 1, 1))
SHAPES = {"n2": (2, 3, 2, None), "n8": (8, 3, 2, None), "t7": (64, 7, 3, None), "n256": (256, 3, 2, None),
          "custom": (8, 4, 3, CUSTOM_EXPS)}


class Statement:
    """a key of known scalars for one shape, and a stock of proof points of known scalars"""

    def __init__(self, oracle, n, t, log_ext, exps=None, seed=1):
        self.n, self.t, self.log_ext, self.e = n, t, log_ext, 1 << log_ext
        self.exps = None if exps is None else [list(row) for row in exps]
        self.g = 0 if exps is None else len(exps)
        assert 3 * t + self.e + 3 + self.g <= 32 and self.e >= t + 1
        self.oracle, self._points = oracle, {}
        rnd = random.Random(977 * seed + n + 31 * t)
        self.ks = GO.shifts(t)
        self.w = NO.domain_root(NO.log2_exact(n))
        self.key_s = [rnd.randrange(1, R) for _ in range(2 * t + 2 + self.g)]
        self.key48 = [self.point(s) for s in self.key_s]
        self.c = types.SimpleNamespace(n=n, t=t, ks=self.ks)
        self.cc = None if exps is None else types.SimpleNamespace(exps=self.exps, t=t, g=self.g, n=n)
        # three sets of proof points (t wires, [z], e - 1 chunks, W)
        self.stock = [[rnd.randrange(1, R) for _ in range(t + self.e + 1)] for _ in range(3)]

    def point(self, s):
        s %= R
        if s not in self._points:
            self._points[s] = TO.g1_scalar(self.oracle, s)
        return self._points[s]

    def member(self, evals, public=(), scalars=None):
        """the proof with the 2 t evaluations (abar, sbar, z(zeta w)) and the points [c]G for c in scalars (t wires, [z], e - 1 chunks,
        W; 0 is the point at infinity)"""
        t, e = self.t, self.e
        scalars = self.stock[0] if scalars is None else list(scalars)
        assert len(evals) == 2 * t and len(scalars) == t + e + 1 and all(0 <= v < R for v in evals)
        proof = b"".join(self.point(s) for s in scalars[:t + e]) + b"".join(TR.fr_bytes(v) for v in evals) + self.point(scalars[-1])
        assert len(proof) == TR.proof_size(t, self.log_ext)
        L = TR.layout(t, self.log_ext)
        assert L["evals"][0] == 48 * (t + e) and L["w"][1] == len(proof)
        return VB.Member(proof, [p % R for p in public], scalars[:t], scalars[t], scalars[t + 1:t + e], scalars[-1])

    def contribution(self, m, five):
        return VB.contribution(self.c, self.log_ext, self.key_s, self.key48, m, self.cc, challenges=five)


_STATEMENTS = {}


def statement(oracle, which):
    if which not in _STATEMENTS:
        _STATEMENTS[which] = Statement(oracle, *SHAPES[which])
    return _STATEMENTS[which]


# ---- the kernels' lanes in plain integers (for the host replay; the constants are free, as the replay takes them) ----------------
def model_public(public, zeta, w, w64, invn, lg_n):
    """(PI(zeta), hit) as k_cvb_public computes them with w^i = w^(i mod 64) (w64)^(i div 64)"""
    wi = [pow(w, i % 64, R) * pow(w64, i // 64, R) % R for i in range(len(public))]
    for i, x in enumerate(wi):
        if x == zeta % R:
            return public[i] % R, i
    acc = sum(p * x % R * pow(zeta - x, -1, R) for p, x in zip(public, wi))
    return acc * (pow(zeta, 1 << lg_n, R) - 1) % R * invn % R, -1


def model_lanes(t, lg_n, e, exps, consts, five, rho, evals, public):
    """what the replay prints for one record: (pi, hit, the four values of k_cvb_lin, [(tag, value)] for the lanes of k_cvb_scalars)"""
    w, w1, invn, w64, ks = consts
    beta, gamma, alpha, zeta, v = five
    g = len(exps) if exps else 0
    abar, sbar, zw = evals[:t], evals[t:2 * t - 1], evals[2 * t - 1]
    pi, hit = model_public(public, zeta, w, w64, invn, lg_n) if public else (0, -1)
    zn = pow(zeta, 1 << lg_n, R)
    l0 = 1 if zeta % R == 1 else (zn - 1) * invn % R * pow(zeta - 1, -1, R) % R
    A, B = 1, zw
    for j in range(t):
        A = A * (abar[j] + gamma + beta * ks[j] % R * zeta) % R
        if j + 1 < t:
            B = B * (abar[j] + gamma + beta * sbar[j]) % R
    a2l = alpha * alpha % R * l0 % R
    sc_z, sc_sig = (alpha * A + a2l) % R, -alpha * B % R * beta % R
    konst = (pi - alpha * B % R * (abar[t - 1] + gamma) - a2l) % R
    lanes = [("s", rho * pow(v, q + 1, R) % R) for q in range(t)] + [("s", rho * sc_z % R)]
    lanes += [("s", rho * -(zn - 1) % R * pow(zn, c, R) % R) for c in range(e - 1)] + [("s", rho * pow(v, 2 * t, R) % R)]
    mzw = -zeta * w % R
    lanes += [("s", mzw), ("s", -zeta % R), ("s", mzw * zeta % R), ("s", zeta * w1 % R)]
    g0 = (konst - sum(pow(v, i, R) * evals[i - 1] for i in range(1, 2 * t))) % R
    g1 = -pow(v, 2 * t, R) * zw % R
    key = abar + [abar[0] * abar[1] % R, 1] + [pow(v, j - 1, R) for j in range(t + 2, 2 * t + 1)] + [sc_sig]
    for row in exps or []:
        m = 1
        for a, p in zip(abar, row):
            m = m * pow(a, p, R) % R
        key.append(m)
    assert len(key) == 2 * t + 2 + g
    lanes += [("r", rho * mzw % R * c % R) for c in key] + [("r", rho * (mzw * g0 - zeta * g1) % R)]
    lanes += [("r", rho * c % R) for c in key] + [("r", rho * (g0 + g1) % R)]
    return pi, hit, [zn, sc_z, sc_sig, konst], lanes
