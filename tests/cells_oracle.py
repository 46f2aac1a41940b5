"""Big-integer references for the cell tests (tests/test_cells*.py): the cells of a domain of N = 2^K points, their
vanishing polynomials X^l - a_j and the stride-l synthetic division, written out in Python integers mod r."""
import ntt_oracle as NO

R = NO.R


def brp(x, bits):
    """bits-bit bit reversal of x"""
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def cell_root(K, t, j):
    """a_j = w_N^(j l): X^l - a_j vanishes on cell j"""
    return pow(NO.domain_root(K), j << t, R)


def cell_points(K, t, j):
    """the l points of cell j: w_N^(j + (N/l) i), i < l"""
    w = NO.domain_root(K)
    return [pow(w, j + (i << (K - t)), R) for i in range(1 << t)]


def vanishing(zs):
    """prod (X - z_i), coefficients low to high"""
    zc = [1]
    for z in zs:
        zc = [((zc[j - 1] if j else 0) - z * (zc[j] if j < len(zc) else 0)) % R for j in range(len(zc) + 1)]
    return zc


def trim(vals):
    v = [x % R for x in vals]
    while v and v[-1] == 0:
        v.pop()
    return v


def stride_quotient(vals, l, a):
    """q with P = q (X^l - a) + rem: q[i] = c[i + l] + a q[i + l], n' - l values (none when n' <= l)"""
    c = trim(vals)
    if len(c) <= l:
        return []
    q = [0] * (len(c) - l)
    for i in range(len(q) - 1, -1, -1):
        q[i] = (c[i + l] + a * (q[i + l] if i + l < len(q) else 0)) % R
    return q


def stride_remainder(vals, l, a, q):
    """rem[i] = c[i] + a q[i] (i < l): the remainder of P by X^l - a"""
    c = [x % R for x in vals] + [0] * l
    return [(c[i] + a * (q[i] if i < len(q) else 0)) % R for i in range(l)]


def poly_eval(vals, x):
    acc = 0
    for c in reversed(vals):
        acc = (acc * x + c) % R
    return acc


def cells(vals, K, t):
    """cell-major values: out[j l + i] = P(w_N^(j + (N/l) i))"""
    ev = NO.ntt([v % R for v in vals] + [0] * ((1 << K) - len(vals)))
    l = 1 << t
    return [ev[j + (i << (K - t))] for j in range((1 << K) >> t) for i in range(l)]


def das_cell(K, t, c):
    """(our cell, value order) of cell c of the bit-reversed list: our cell brp_(K-t)(c), position i at brp_t(i)"""
    return brp(c, K - t), [brp(i, t) for i in range(1 << t)]
