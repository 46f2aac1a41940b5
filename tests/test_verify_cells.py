"""CPU: the algebra of kzg_verify_cells_batch (tests/verify_cells_oracle.py) with the known secret --
the right side is exactly [s^l] times the left for valid batches and differs after each corruption -- the G1 subgroup test
against the order test, and the a + b lambda weights."""
import os
import random
import re

import pytest

import bigint_twin as T
import cells_oracle as CO
import ntt_oracle as NO
import verify_cells_oracle as VO

R = NO.R
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kzg_poly_commit_exploration_amd", "csrc")
S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)


def _batch(rnd, K, t, polys, n):
    """every cell of `polys` random polynomials as records over discrete logarithms: (commitments, idx, ids, values, proofs)"""
    l, M = 1 << t, (1 << K) >> t
    coms, idx, ids, vals, prfs = [], [], [], [], []
    for b in range(polys):
        c = [rnd.randrange(R) for _ in range(n)]
        coms.append(CO.poly_eval(c, S))
        cells = CO.cells(c, K, t)
        for j in range(M):
            a = CO.cell_root(K, t, j)
            v = cells[j * l:(j + 1) * l]
            I_s = CO.poly_eval(VO.interpolant(K, t, j, v), S)
            idx.append(b)
            ids.append(j)
            vals.append(v)
            prfs.append((coms[b] - I_s) * pow(pow(S, l, R) - a, -1, R) % R)
    return coms, idx, ids, vals, prfs


def _holds(K, t, coms, idx, ids, vals, prfs, weights):
    lhs, rhs = VO.scalar_sides(K, t, coms, idx, ids, vals, prfs, weights, S)
    return rhs == pow(S, 1 << t, R) * lhs % R


def test_interpolant_matches_the_cell_values():
    rnd = random.Random(1)
    K, t = 5, 3
    c = [rnd.randrange(R) for _ in range(20)]
    cells = CO.cells(c, K, t)
    for j in range(4):
        I = VO.interpolant(K, t, j, cells[8 * j:8 * j + 8])
        assert [CO.poly_eval(I, x) for x in CO.cell_points(K, t, j)] == cells[8 * j:8 * j + 8]


@pytest.mark.parametrize("t", range(7))
def test_known_secret_every_cell_size(t):
    rnd = random.Random(10 + t)
    K = t + 2
    coms, idx, ids, vals, prfs = _batch(rnd, K, t, 2, min(50, 1 << K))
    k = len(ids)
    w = [VO.glv_weight(rnd.getrandbits(64), rnd.getrandbits(64)) for _ in range(k)]
    assert _holds(K, t, coms, idx, ids, vals, prfs, w)
    order = list(range(k)) + [0, 1]  # shuffled with duplicates
    rnd.shuffle(order)
    pick = lambda a: [a[i] for i in order]  # noqa: E731
    w2 = [VO.glv_weight(rnd.getrandbits(64), rnd.getrandbits(64)) for _ in order]
    assert _holds(K, t, coms, pick(idx), pick(ids), pick(vals), pick(prfs), w2)
    # corruptions: a value, two proofs swapped, another commitment, another cell id, a proof or a commitment shifted by G
    v2 = [list(v) for v in vals]
    v2[1][0] = (v2[1][0] + 1) % R
    assert not _holds(K, t, coms, idx, ids, v2, prfs, w)
    p2 = list(prfs)
    p2[0], p2[2] = p2[2], p2[0]
    assert prfs[0] == prfs[2] or not _holds(K, t, coms, idx, ids, vals, p2, w)
    i2 = list(idx)
    i2[0] = 1 - i2[0]
    assert not _holds(K, t, coms, i2, ids, vals, prfs, w)
    M = (1 << K) >> t
    j2 = list(ids)
    j2[0] = (j2[0] + 1) % M
    assert not _holds(K, t, coms, idx, j2, vals, prfs, w)
    p3 = list(prfs)
    p3[k - 1] = (p3[k - 1] + 1) % R
    assert not _holds(K, t, coms, idx, ids, vals, p3, w)
    c3 = [(coms[0] + 1) % R] + coms[1:]
    assert not _holds(K, t, c3, idx, ids, vals, prfs, w)


def test_all_records_of_one_cell():
    rnd = random.Random(3)
    K, t = 6, 2
    coms, idx, ids, vals, prfs = _batch(rnd, K, t, 3, 40)
    rows = [i for i, j in enumerate(ids) if j == 7] * 5
    w = [rnd.randrange(R) for _ in rows]
    assert _holds(K, t, coms, [idx[i] for i in rows], [ids[i] for i in rows], [vals[i] for i in rows],
                  [prfs[i] for i in rows], w)


def _non_g1_points(seed, count):
    rnd = random.Random(seed)
    out = []
    while len(out) < count:
        x = rnd.randrange(T.P)
        y2 = (x * x * x + 4) % T.P
        if pow(y2, (T.P - 1) // 2, T.P) == 1:
            out.append((x, pow(y2, (T.P + 1) // 4, T.P)))
    return out


def test_subgroup_test_agrees_with_the_order():
    rnd = random.Random(4)
    g1 = [T.INF, T.G1] + [T.g1_mul(T.G1, rnd.randrange(1, R)) for _ in range(3)]
    for pt in g1:
        assert VO.g1_in_subgroup(pt) and VO.g1_in_subgroup_by_order(pt)
    for pt in _non_g1_points(5, 4):
        assert T.g1_is_on_curve(pt)
        assert not VO.g1_in_subgroup(pt) and not VO.g1_in_subgroup_by_order(pt)
    # the other cube root (the one fq_beta() holds, which pairs with z^2 - 1) gives [lambda] P, a different statement
    assert T.g1_mul(T.G1, VO.LAMBDA) == (VO.BETA * T.G1[0] % T.P, T.G1[1])
    assert VO.BETA2 == (T.P - 1 - VO.BETA) % T.P


def test_glv_weights_are_distinct_and_below_r():
    assert (VO.LAMBDA * VO.LAMBDA + VO.LAMBDA + 1) % R == 0
    assert VO.LAMBDA < 1 << 128 and (1 << 64) * VO.LAMBDA < R
    rnd = random.Random(5)
    seen = {}
    for _ in range(2000):
        a, b = rnd.getrandbits(64), rnd.getrandbits(64)
        w = VO.glv_weight(a, b)
        assert w == a + b * VO.LAMBDA < R  # no reduction: (a, b) -> w is injective
        assert seen.setdefault(w, (a, b)) == (a, b)
    for a, b in ((0, 0), (2**64 - 1, 2**64 - 1), (2**64 - 1, 0), (0, 2**64 - 1)):
        assert VO.glv_weight(a, b) == a + b * VO.LAMBDA < R


def test_beta_digits_match_fk20_and_the_oracle():
    """verify_kernels.hip restates fk20_kernels.hip's GLV ladder: the same digits of beta, which the oracle holds too"""
    digits = []
    for name in ("fk20_kernels.hip", "verify_kernels.hip"):
        body = re.search(r"constexpr int32_t B\[13\] = \{([^}]*)\}", open(os.path.join(CSRC, name)).read()).group(1)
        digits.append([int(x.strip(), 16) if not x.strip().startswith("-") else -int(x.strip()[1:], 16) for x in body.split(",")])
    assert digits[0] == digits[1] == VO._BETA_DIGITS
