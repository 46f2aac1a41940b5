"""CPU: the coset erasure decode of tests/recover_oracle.py (the reference of kzg_recover_cells_and_proofs) against Lagrange
interpolation from the received points, and the identities it rests on."""
import random

import pytest

import cells_oracle as CO
import ntt_oracle as NO
import recover_oracle as RO

R = NO.R


def _case(rnd, K, t, n, k):
    """a random polynomial of n coefficients, k random received cells in shuffled order and their values"""
    N, l = 1 << K, 1 << t
    M = N >> t
    c = [rnd.randrange(R) for _ in range(n)]
    cells = CO.cells(c, K, t)
    ids = rnd.sample(range(M), k)
    return c, ids, [cells[j * l:(j + 1) * l] for j in ids]


def _lagrange_check(K, t, n, ids, received, want):
    """any n of the received points determine P: interpolate from them independently"""
    pts = [(x, y) for j, vals in zip(ids, received) for x, y in zip(CO.cell_points(K, t, j), vals)]
    xs, ys = zip(*pts[:n])
    assert RO.lagrange(list(xs), list(ys)) == want


def _shapes():
    rnd = random.Random(9)
    out = []
    for K in range(0, 7):
        for t in range(0, K + 1):
            N, l = 1 << K, 1 << t
            M = N >> t
            n = rnd.randrange(1, N + 1)
            k = rnd.randrange(-(-n // l), M + 1)
            out.append((K, t, n, k))
    return out


@pytest.mark.parametrize("K,t,n,k", _shapes())
def test_decode_random_shapes(K, t, n, k):
    rnd = random.Random(K * 100 + t * 10 + n)
    c, ids, received = _case(rnd, K, t, n, k)
    got, ok = RO.decode(n, K, t, ids, received)
    assert ok and got == c
    _lagrange_check(K, t, n, ids, received, c)


@pytest.mark.parametrize("K,t", [(0, 0), (3, 0), (4, 2), (5, 5), (6, 3), (6, 6)])
def test_minimal_k_decodes_anything(K, t):
    """k l = n: every set of values is a codeword, and the decode interpolates it"""
    rnd = random.Random(K + t)
    l = 1 << t
    M = (1 << K) >> t
    k = max(1, M // 2)
    n = k * l
    ids = rnd.sample(range(M), k)
    received = [[rnd.randrange(R) for _ in range(l)] for _ in ids]
    got, ok = RO.decode(n, K, t, ids, received)
    assert ok
    _lagrange_check(K, t, n, ids, received, got)
    # and back: its cells at the received positions are the input
    cells = CO.cells(got, K, t)
    for j, vals in zip(ids, received):
        assert cells[j * l:(j + 1) * l] == vals


@pytest.mark.parametrize("K,t", [(3, 1), (6, 0), (6, 6)])
def test_all_cells_received(K, t):
    rnd = random.Random(7 * K + t)
    M = (1 << K) >> t
    n = 1 << K
    c, ids, received = _case(rnd, K, t, n, M)
    assert RO.missing_cells(K, t, ids) == []
    got, ok = RO.decode(n, K, t, ids, received)
    assert ok and got == c


def test_shuffled_ids_give_the_same_result():
    rnd = random.Random(3)
    K, t, n = 6, 2, 32
    c, ids, received = _case(rnd, K, t, n, 10)
    order = list(range(len(ids)))
    rnd.shuffle(order)
    got, ok = RO.decode(n, K, t, [ids[i] for i in order], [received[i] for i in order])
    assert ok and got == c


@pytest.mark.parametrize("K,t,n,k", [(4, 0, 8, 9), (6, 2, 32, 9), (6, 3, 20, 4), (5, 5, 16, 1)])
def test_corrupted_value_is_caught(K, t, n, k):
    """one extra cell of redundancy at least: a changed value leaves non-zero coefficients at [n, N)"""
    rnd = random.Random(K * t + n)
    l = 1 << t
    assert k * l > n
    c, ids, received = _case(rnd, K, t, n, k)
    s, i = rnd.randrange(k), rnd.randrange(l)
    received[s][i] = (received[s][i] + 1 + rnd.randrange(R - 1)) % R
    _, ok = RO.decode(n, K, t, ids, received)
    assert not ok


@pytest.mark.parametrize("K,t", [(4, 1), (6, 3), (6, 0), (3, 3)])
def test_vanishing_identities(K, t):
    """Z(X) = Z'(X^l) vanishes on exactly the missing points; Z' has no zero on the coset g^l <w_M>"""
    rnd = random.Random(K * 8 + t)
    l = 1 << t
    M = (1 << K) >> t
    ids = rnd.sample(range(M), rnd.randrange(0, M + 1))
    missing = RO.missing_cells(K, t, ids)
    z = RO.vanishing_full(K, t, missing)
    zp = RO.vanishing_prime(K, t, missing)
    w = NO.domain_root(K)
    for e in range(1 << K):
        x = pow(w, e, R)
        assert CO.poly_eval(z, x) == CO.poly_eval(zp, pow(x, l, R))
        assert (CO.poly_eval(z, x) == 0) == (e % M in missing)
    gl = pow(RO.G, l, R)
    wm = NO.domain_root(K - t)
    assert all(CO.poly_eval(zp, gl * pow(wm, i, R) % R) != 0 for i in range(M))
    # g^l is no M-th root of unity and g w_N^e never lies in the domain
    assert pow(gl, M, R) != 1 and pow(RO.G, 1 << K, R) != 1
