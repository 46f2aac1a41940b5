"""Independent references for the Lagrange-basis entry points (kzg_lagrange_*, kzg_commit_lagrange, kzg_open_lagrange,
kzg_quotient_lagrange), in Python integers mod r.

Domain of n = 2^k points {w^i}, w = ntt_oracle.domain_root(k), natural order.
  * lagrange_at       l_i(s) = w^i (s^n - 1) / (n (s - w^i)) for every i, with the in-domain limit: for s = w^m it is 1 at
                      i = m and 0 elsewhere.  [l_i(S)]G is point i of the basis of the setup with secret S.
  * quotient_evals    the values of (P - y) / (X - z) over the domain, straight from the values of P:
                      q_i = (f_i - y) / (w^i - z) where w^i != z, and for z = w^m the missing entry from the others,
                      q_m = -sum_{i != m} q_i w^(i - m): the quotient has degree <= n - 2, so its coefficient of X^(n-1),
                      (1/n) sum_i q_i w^(-i (n-1)) = (1/n) sum_i q_i w^i, vanishes.
  * brp / bit_reverse the bit-reversal permutation the ceremony files order g1_lagrange by.
"""
import ntt_oracle as NO

R = NO.R


def domain(k):
    w = NO.domain_root(k)
    pts = [1] * (1 << k)
    for i in range(1, len(pts)):
        pts[i] = pts[i - 1] * w % R
    return pts


def lagrange_at(k, s):
    """[l_0(s), ..., l_(n-1)(s)]"""
    n = 1 << k
    s %= R
    pts = domain(k)
    if s in pts:  # the limit: l_i(w^m) = [i == m]
        m = pts.index(s)
        return [1 if i == m else 0 for i in range(n)]
    inv = NO.batch_inverse([n * (s - p) % R for p in pts])
    num = (pow(s, n, R) - 1) % R
    return [p * num % R * d % R for p, d in zip(pts, inv)]


def quotient_evals(evals, z, y):
    """the n values of (P - y) / (X - z) for the claim y = P(z) (a wrong y has no polynomial quotient: the caller must not
    ask), z inside or outside the domain"""
    n = len(evals)
    k = NO.log2_exact(n)
    z %= R
    pts = domain(k)
    m = pts.index(z) if z in pts else None
    inv = NO.batch_inverse([(p - z) % R if i != m else 1 for i, p in enumerate(pts)])
    q = [(f - y) * d % R for f, d in zip(evals, inv)]
    if m is not None:
        winv = pow(pts[m], R - 2, R)
        q[m] = 0
        q[m] = -sum(qi * p for qi, p in zip(q, pts)) * winv % R
    return q


def brp(i, k):
    return int(format(i, "0%db" % k)[::-1], 2) if k else 0


def bit_reverse(items):
    """out[i] = items[brp(i)]: its own inverse"""
    k = NO.log2_exact(len(items))
    return [items[brp(i, k)] for i in range(len(items))]
