"""The lookup circuits the tests of DESIGN.md section 4.26 share: a satisfied circuit of circuit_oracle with a lookup selector q_K in
{0, 1}, and a shuffled table of n rows holding the looked-up tuples, the zero tuple (what a row with q_K = 0 looks up) and
duplicate rows as padding.  Every case is built once, kept and left unchanged.

SHAPES are (n, t, c, log_ext), the smallest where each path changes:
    (1, 2, 1, 2)      w = 1, one opening point          (2, 3, 2, 2)
    (8, 3, 3, 2)                                        (256, 3, 2, 2)    n = kPqTile, N below the LDS transform
    (512, 3, 3, 2)    one kLuTile, N = 2^11             (2048, 3, 2, 2)   one kCombineTile
    (4096, 2, 1, 2)   two tiles, e set by the lookup    (64, 6, 1, 3)     exactly 32 columns at zeta
"""
import random

import circuit_lookup_oracle as CL
import circuit_oracle as CO
import ntt_oracle as NO

R = CL.R
THETA = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
BETA = 0x1F2E3D4C5B6A79881F2E3D4C5B6A7988 % R
GAMMA = 0x123456789ABCDEF0FEDCBA9876543210 % R
ALPHA = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % R

SHAPES = [(1, 2, 1, 2), (2, 3, 2, 2), (8, 3, 3, 2), (256, 3, 2, 2), (512, 3, 3, 2), (2048, 3, 2, 2), (4096, 2, 1, 2), (64, 6, 1, 3)]

_CACHE = {}


def memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def build(n, t, c, with_pi=True):
    """a LookupCircuit whose every row holds, lookups included"""
    k = NO.log2_exact(n)
    circ = CO.satisfied(k, t, 300 + n + 7 * t + c, with_pi)
    rnd = random.Random(9000 + 131 * n + 17 * t + c)
    if n == 1:
        q_k = [1]
    elif n == 2:
        q_k = [0, 1]
    else:
        q_k = [1 if i % 3 == 1 else 0 for i in range(n)]
    rows = []
    for i in range(n):
        tup = tuple(circ.wires[j][i] for j in range(c)) if q_k[i] else (0,) * c
        if tup not in rows:
            rows.append(tup)
    if 0 in q_k and (0,) * c not in rows:
        rows.append((0,) * c)
    assert len(rows) <= n
    while len(rows) < n:
        rows.append(rows[rnd.randrange(len(rows))])  # padding: duplicates
    if n == 2:
        rows.reverse()  # (in row order the folded table would equal the folded lookups: G' = 0, a vacuous case)
    else:
        rnd.shuffle(rows)
    table = [[row[j] for row in rows] for j in range(c)]
    lc = CL.LookupCircuit(circ, table, q_k)
    f, T, m, phi, last, missing = CL.columns(lc, THETA, BETA)
    assert missing is None and last == 0
    if n >= 2:
        assert f != T
    if n >= 4:
        assert 0 in q_k and 1 in q_k
        assert any(v >= 2 for v in m) and any(v == 0 for v in m)
        assert any(v != 0 for v in phi)
    return lc


class Case:
    """lc, the per-proof columns f, T, m, phi over H, the accumulator z and the quotient T_q under the module's challenges"""

    def __init__(self, n, t, c, log_ext, with_pi):
        self.n, self.t, self.c, self.log_ext = n, t, c, log_ext
        self.lc = build(n, t, c, with_pi)
        self.f, self.T, self.m, self.phi, last, _ = CL.columns(self.lc, THETA, BETA)
        assert last == 0
        self.z, zlast = CO.z_of(self.lc.circuit, BETA, GAMMA)
        assert zlast == 1
        self._q = None

    @property
    def gprime(self):
        return memo(("gprime", id(self)), lambda: CL.gprime_coeffs(self.lc, THETA, BETA, ALPHA, self.m, self.phi))

    @property
    def quotient(self):
        if self._q is None:
            self._q = CO.quotient(self.lc.circuit, self.z, ALPHA, BETA, GAMMA, extra=self.gprime)
        return self._q


def case(n, t, c, log_ext, with_pi=True):
    return memo(("case", n, t, c, log_ext, with_pi), lambda: Case(n, t, c, log_ext, with_pi))
