"""The custom circuits the tests of DESIGN.md section 4.27 share: a satisfied circuit of circuit_oracle with g random selector
columns qx_s, each nonzero on about a third of the rows (n >= 4) and zero elsewhere, and q_C lowered row by row by
sum_s qx_s prod_j f_j^p[s][j], so that the witness and the permutation stay as they are.  Every case is built once, kept and left
unchanged.

SHAPES are (n, t, log_ext, exponents), the smallest where each path changes:
    (1, 2, 2, [[2,0]])                  w = 1, one opening point
    (2, 3, 2, [[1,1,1],[3,0,0]])        d_max = e - 1
    (8, 3, 3, [[5,0,0],[0,2,1]])        the S-box x^5; d_max > t, so the blinded rule is the new one
    (8, 3, 3, [[7,0,0]])                plain allowed, blinded REFUSED: 7 n + 7 > L_T
    (256, 3, 2, [[0,0,3]])              n = kPqTile
    (2048, 3, 2, [[2,0,0],[0,1,1]])     one kCombineTile
    (4096, 2, 2, [[2,1],[1,2]])         two tiles; blinded at 3 n + 3 <= L_T
    (64, 6, 3, three terms, d_max = 7)  exactly 32 columns at zeta
"""
import random

import blind_oracle as BO
import circuit_custom_oracle as CX
import circuit_oracle as CO
import ntt_oracle as NO

R = CX.R
BETA = 0x1F2E3D4C5B6A79881F2E3D4C5B6A7988 % R
GAMMA = 0x123456789ABCDEF0FEDCBA9876543210 % R
ALPHA = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % R

SBOX = (8, 3, 3, ((5, 0, 0), (0, 2, 1)))
REFUSED_BLINDED = (8, 3, 3, ((7, 0, 0),))
WIDE = (64, 6, 3, ((2, 1, 1, 1, 1, 1), (0, 0, 3, 0, 0, 0), (1, 0, 0, 0, 0, 2)))
SHAPES = [(1, 2, 2, ((2, 0),)), (2, 3, 2, ((1, 1, 1), (3, 0, 0))), SBOX, REFUSED_BLINDED, (256, 3, 2, ((0, 0, 3),)),
          (2048, 3, 2, ((2, 0, 0), (0, 1, 1))), (4096, 2, 2, ((2, 1), (1, 2))), WIDE]

_CACHE = {}


def memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def d_max(exps):
    return max(sum(row) for row in exps)


def blinded_legal(n, t, log_ext, exps):
    return CX.blinded_ok(n, t, log_ext, d_max(exps))


# ---- what the table above claims of each shape, checked here on the CPU ----
for _n, _t, _le, _ex in SHAPES:
    assert CX.shape_ok(_t, _le, [list(r) for r in _ex]), (_n, _t, _le, _ex)
assert d_max(SHAPES[1][3]) == (1 << SHAPES[1][2]) - 1
assert d_max(SBOX[3]) > SBOX[1] and blinded_legal(*SBOX) and BO.shape_ok(SBOX[0], SBOX[1], SBOX[2])
assert not blinded_legal(*REFUSED_BLINDED) and BO.shape_ok(8, 3, 3) and 7 * 8 + 7 > BO.quotient_len(8, 3, 3)
assert SHAPES[4][0] == 256 and SHAPES[5][0] == 2048 and SHAPES[6][0] == 2 * 2048
assert blinded_legal(*SHAPES[6]) and CX.blinded_keep(4096, 2, 3) == 3 * 4096 + 3 <= BO.quotient_len(4096, 2, 2)
assert 3 * WIDE[1] + (1 << WIDE[2]) + 3 + len(WIDE[3]) == CX.LIN_MAX_COLUMNS and d_max(WIDE[3]) == 7 and blinded_legal(*WIDE)
BLINDED_SHAPES = [s for s in SHAPES if blinded_legal(*s)]
assert [s[0] for s in BLINDED_SHAPES] == [8, 256, 2048, 4096, 64]  # (n = 1, 2: N < t n + t + 4, the rule of section 4.24)


def build(n, t, exps, with_pi=True):
    """a CustomCircuit whose every row holds, custom terms included"""
    k = NO.log2_exact(n)
    g = len(exps)
    circ = CO.satisfied(k, t, 500 + n + 7 * t + 3 * g + d_max(exps), with_pi)
    rnd = random.Random(11000 + 131 * n + 17 * t + g)
    if n >= 4:
        qx = [[rnd.randrange(1, R) if (i + s) % 3 == 1 else 0 for i in range(n)] for s in range(g)]
    else:
        qx = [[rnd.randrange(1, R) for _ in range(n)] for _ in range(g)]
    cc = CX.CustomCircuit(circ, qx, [list(r) for r in exps])
    gp = CX.gprime_rows(cc)
    circ.q_const = [(a - b) % R for a, b in zip(circ.q_const, gp)]
    assert CX.gate_rows(cc) == [0] * n
    if n >= 4:
        for s in range(g):  # every term is nonzero on some row
            one = CX.CustomCircuit(circ, [qx[s]], [list(exps[s])])
            assert any(CX.gprime_rows(one)), s
        assert any(gp)  # G' is not the zero polynomial
        assert any(CO.gate_rows(circ))  # the base gate alone does NOT hold: the case is not vacuous
    return cc


class Case:
    """cc, the accumulator z and, lazily, the plain coefficients and quotient under the module's challenges"""

    def __init__(self, n, t, log_ext, exps, with_pi):
        self.n, self.t, self.log_ext, self.exps = n, t, log_ext, exps
        self.cc = build(n, t, exps, with_pi)
        self.z, zlast = CO.z_of(self.cc.circuit, BETA, GAMMA)
        assert zlast == 1

    @property
    def zero(self):
        return BO.Blinders.zero(self.t, self.log_ext)

    @property
    def coefs(self):
        return memo(("coefs", id(self)), lambda: CX.coefficients(self.cc, self.z, self.zero))

    @property
    def gprime(self):
        return memo(("gprime", id(self)), lambda: CX.gprime_coeffs(self.cc))

    @property
    def quotient(self):
        """T padded to L_T; its first N - n coefficients are what the plain call returns"""
        return memo(("T", id(self)), lambda: CX.quotient(self.cc, self.coefs, self.log_ext, self.zero, ALPHA, BETA, GAMMA, z=self.z))

    def blinders(self, seed=1):
        return BO.Blinders.random(self.t, self.log_ext, seed + self.n)

    def blinded(self, seed=1):
        """(bl, coefs, T~) under the module's challenges"""
        def make():
            bl = self.blinders(seed)
            coefs = CX.coefficients(self.cc, self.z, bl)
            return bl, coefs, CX.quotient(self.cc, coefs, self.log_ext, bl, ALPHA, BETA, GAMMA)
        return memo(("blinded", id(self), seed), make)


def case(n, t, log_ext, exps, with_pi=True):
    return memo(("case", n, t, log_ext, exps, with_pi), lambda: Case(n, t, log_ext, exps, with_pi))
