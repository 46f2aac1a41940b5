"""CPU: the algebra behind kzg_cells_and_proofs (tests/cells_oracle.py) -- the stride-l division by X^l - a_j is the
division by the cell's vanishing polynomial, and the bit-reversed cell order of sampling specs maps onto this API's."""
import random

import pytest

import cells_oracle as CO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import open_points_oracle as PO

R = CO.R
SHAPES = [(64, 7, 0), (64, 7, 3), (128, 7, 6), (100, 8, 2), (300, 9, 4), (65, 6, 6), (70, 7, 6)]


def _poly(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R) for _ in range(n)]


@pytest.mark.parametrize("n,K_,t", SHAPES)
def test_stride_division_is_division_by_the_cell_vanishing_polynomial(n, K_, t):
    c = _poly(n, n * 7 + K_ + t)
    for j in sorted({0, 1, ((1 << K_) >> t) - 1, ((1 << K_) >> t) // 2}):
        zs = CO.cell_points(K_, t, j)
        a = CO.cell_root(K_, t, j)
        q = CO.stride_quotient(c, 1 << t, a)
        want_q, want_rem = PO.poly_div_vanishing(c, zs)
        assert q == want_q
        rem = CO.stride_remainder(c, 1 << t, a, q)
        assert CO.trim(rem) == CO.trim(want_rem)
        for z in zs:  # the remainder interpolates P on the coset
            assert CO.poly_eval(rem, z) == CO.poly_eval(c, z)


@pytest.mark.parametrize("K_,t", [(1, 0), (3, 1), (7, 3), (8, 6), (13, 6), (13, 0)])
def test_vanishing_polynomial_of_a_cell(K_, t):
    l = 1 << t
    for j in sorted({0, 1, ((1 << K_) >> t) - 1}):
        z = CO.vanishing(CO.cell_points(K_, t, j))
        assert z == [(-CO.cell_root(K_, t, j)) % R] + [0] * (l - 1) + [1]
        assert CO.cell_root(K_, t, j) == pow(NO.domain_root(K_ - t), j, R)


def test_trailing_zeros_and_short_polynomials():
    c = _poly(40, 1) + [0] * 30
    a = CO.cell_root(7, 3, 5)
    assert CO.stride_quotient(c, 8, a) == PO.poly_div_vanishing(c, CO.cell_points(7, 3, 5))[0]
    assert len(CO.stride_quotient(c, 8, a)) == 32
    assert CO.stride_quotient(_poly(8, 2), 8, a) == [] and CO.stride_quotient([], 8, a) == []


def test_bit_reversed_cells_map_onto_natural_cells():
    for K_ in range(0, 14):
        N = 1 << K_
        for t in range(0, min(6, K_) + 1):
            l = 1 << t
            for c in range(N >> t):
                j, order = CO.das_cell(K_, t, c)
                for i in range(l):  # DAS position c l + i holds evaluation index brp_K(c l + i)
                    assert CO.brp(c * l + i, K_) == j + (order[i] << (K_ - t))


def test_cells_gather_matches_the_domain_points():
    c = _poly(50, 3)
    K_, t = 7, 2
    got = CO.cells(c, K_, t)
    for j in (0, 3, 31):
        for i, z in enumerate(CO.cell_points(K_, t, j)):
            assert got[j * 4 + i] == CO.poly_eval(c, z)


def test_library_exports_the_cell_symbols():
    lib = K.load_library()
    for name in ("kzg_cells_and_proofs", "kzg_cells_and_proofs_evaluations", "kzg_quotient_cells"):
        assert hasattr(lib, name) and name in K.ABI_SYMBOLS
