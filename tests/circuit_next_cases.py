"""The next-row circuits the tests of DESIGN.md section 4.28 share: a satisfied circuit of circuit_oracle with g random selector
columns qx_s, each nonzero on about a third of the rows (n >= 4) and zero elsewhere -- the first term with a next-row exponent also
on row n - 1, whose next row is row 0 -- and q_C lowered row by row by sum_s qx_s[i] prod_j f_j[i]^p[s][j] f_j[i+1]^p'[s][j], so
that the witness and the permutation stay as they are.  Every case is built once, kept and left unchanged.

SHAPES are (n, t, log_ext, p, p'), the smallest where each part can go wrong:
    (2, 2, 2, [[1,0]], [[0,1]])                          N = 8: one partial workgroup, the wrap inside it
    (8, 3, 2, [[1,0,0],[0,0,0]], [[0,1,0],[0,0,2]])      the second term is next-row only; rho = 2
    (8, 3, 3, [[3,0,0]], [[4,0,0]])                      d_max = 7; one wire at both rows
    (64, 3, 2, [[0,0,0],[0,1,1]], [[1,0,0],[0,0,0]])     the accumulator acc' = acc + a b; N = 256, exactly one workgroup
    (2048, 3, 2, [[1,0,0],[0,1,0]], [[0,1,0],[0,0,1]])   32 workgroups, the wrap in the last; one k_lin_combine tile
    (4096, 2, 2, [[1,1]], [[1,0]])                       two tiles
    (64, 6, 3, three terms, d_max = 7, rho = 6)          32 columns at zeta, 7 at zeta w
"""
import random

import circuit_custom_oracle as CX
import circuit_next_oracle as CN
import circuit_oracle as CO
import ntt_oracle as NO

R = CN.R
BETA = 0x1F2E3D4C5B6A79881F2E3D4C5B6A7988 % R
GAMMA = 0x123456789ABCDEF0FEDCBA9876543210 % R
ALPHA = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % R

TINY = (2, 2, 2, ((1, 0),), ((0, 1),))
NEXT_ONLY = (8, 3, 2, ((1, 0, 0), (0, 0, 0)), ((0, 1, 0), (0, 0, 2)))
BOTH_ROWS = (8, 3, 3, ((3, 0, 0),), ((4, 0, 0),))
ACCUMULATOR = (64, 3, 2, ((0, 0, 0), (0, 1, 1)), ((1, 0, 0), (0, 0, 0)))
ONE_TILE = (2048, 3, 2, ((1, 0, 0), (0, 1, 0)), ((0, 1, 0), (0, 0, 1)))
TWO_TILES = (4096, 2, 2, ((1, 1),), ((1, 0),))
WIDE = (64, 6, 3, ((2, 1, 0, 0, 0, 0), (0, 0, 1, 0, 0, 0), (1, 0, 0, 0, 0, 0)),
        ((0, 0, 1, 1, 1, 1), (0, 0, 0, 2, 0, 0), (1, 1, 0, 0, 0, 1)))
SHAPES = [TINY, NEXT_ONLY, BOTH_ROWS, ACCUMULATOR, ONE_TILE, TWO_TILES, WIDE]
SMALL = [TINY, NEXT_ONLY, BOTH_ROWS, ACCUMULATOR]  # the four smallest: what the CPU tests prove and verify, with WIDE

_CACHE = {}


def memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def d_max(exps, exps_next):
    return max(sum(a) + sum(b) for a, b in zip(exps, exps_next))


def rho(exps_next):
    return len(CN.next_wires(exps_next))


# ---- what the table above claims of each shape, checked here on the CPU ----
for _n, _t, _le, _ex, _en in SHAPES:
    assert CN.shape_ok(_n, _t, _le, _ex, _en), (_n, _t, _le, _ex, _en)
assert TINY[0] << TINY[2] == 8
assert not any(NEXT_ONLY[3][1]) and rho(NEXT_ONLY[4]) == 2
assert d_max(BOTH_ROWS[3], BOTH_ROWS[4]) == 7 and BOTH_ROWS[3][0][0] and BOTH_ROWS[4][0][0]
assert ACCUMULATOR[0] << ACCUMULATOR[2] == 256
assert (ONE_TILE[0] << ONE_TILE[2]) == 32 * 256 and ONE_TILE[0] == 2048 and TWO_TILES[0] == 2 * 2048
assert 3 * WIDE[1] + (1 << WIDE[2]) + 3 + len(WIDE[3]) == CX.LIN_MAX_COLUMNS and d_max(WIDE[3], WIDE[4]) == 7 and rho(WIDE[4]) == 6
assert 1 + rho(WIDE[4]) == 7  # the columns at zeta w: z and the wires of R


def build(n, t, exps, exps_next, with_pi=True):
    """a NextCircuit whose every row holds, next-row terms included"""
    k = NO.log2_exact(n)
    g = len(exps)
    circ = CO.satisfied(k, t, 900 + n + 7 * t + 3 * g + d_max(exps, exps_next), with_pi)
    rnd = random.Random(23000 + 131 * n + 17 * t + g)
    if n >= 4:
        qx = [[rnd.randrange(1, R) if (i + s) % 3 == 1 else 0 for i in range(n)] for s in range(g)]
        first_next = next(s for s in range(g) if any(exps_next[s]))
        qx[first_next][n - 1] = rnd.randrange(1, R)  # the term of row n - 1 reads row 0
    else:
        qx = [[rnd.randrange(1, R) for _ in range(n)] for _ in range(g)]
    nc = CN.NextCircuit(circ, qx, [list(r) for r in exps], [list(r) for r in exps_next])
    gp = CN.gprime_rows(nc)
    circ.q_const = [(a - b) % R for a, b in zip(circ.q_const, gp)]
    assert CN.gate_rows(nc) == [0] * n
    if n >= 4:
        zeros = [[0] * t for _ in range(g)]
        for s in range(g):  # every term is nonzero on some row
            one = [qx[j] if j == s else [0] * n for j in range(g)]
            assert any(CN.gprime_rows(nc, q_custom=one)), s
        wrap = [[col[i] if i == n - 1 and any(exps_next[s]) else 0 for i in range(n)] for s, col in enumerate(qx)]
        assert CN.gprime_rows(nc, q_custom=wrap)[n - 1] != 0  # some term with p' != 0 is nonzero on row n - 1: the wrap is exercised
        assert any(CO.gate_rows(circ))  # the base gate alone does NOT hold
        dropped = CN.gprime_rows(nc, exps_next=zeros)  # the statement of section 4.27 with the same p
        assert any((a + b) % R for a, b in zip(CO.gate_rows(circ), dropped))  # ... does not hold either
    return nc


class Case:
    """nc, the accumulator z and, lazily, the coefficients and the quotient under the module's challenges"""

    def __init__(self, n, t, log_ext, exps, exps_next, with_pi):
        self.n, self.t, self.log_ext, self.exps, self.exps_next = n, t, log_ext, exps, exps_next
        self.nc = build(n, t, exps, exps_next, with_pi)
        self.z, zlast = CO.z_of(self.nc.circuit, BETA, GAMMA)
        assert zlast == 1

    @property
    def coefs(self):
        return memo(("coefs", id(self)), lambda: CN.coefficients(self.nc, self.z, self.log_ext))

    @property
    def gprime(self):
        return memo(("gprime", id(self)), lambda: CN.gprime_coeffs(self.nc))

    @property
    def quotient(self):
        """T padded to L_T; its first N - n coefficients are what the call returns"""
        return memo(("T", id(self)), lambda: CN.quotient(self.nc, self.z, self.log_ext, ALPHA, BETA, GAMMA))


def case(n, t, log_ext, exps, exps_next, with_pi=True):
    return memo(("case", n, t, log_ext, exps, exps_next, with_pi), lambda: Case(n, t, log_ext, exps, exps_next, with_pi))
