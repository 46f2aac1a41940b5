"""Independent references for the log-derivative lookup entry points (kzg_logderivative_sum, kzg_lookup_sum, kzg_lookup_commit,
kzg_batch_inverse, kzg_lookup_multiplicities), in Python integers mod r.

t numerator columns a_j and t denominator columns b_j of n values each (lists of t lists; nums None: every numerator is one).
  * direct            phi_0 = 0, phi_(i+1) = phi_i + sum_j a_j[i] / b_j[i] with one modular inverse per fraction: the
                      definition, for small n
  * row_pairs         (N_i, D_i) with N_i / D_i = sum_j a_j[i] / b_j[i], by cross-multiplication: no inversion
  * check             no inversion at all: phi_0 = 0 and (phi_(i+1) - phi_i) D_i = N_i for every i (phi_n = last).  With no D_i
                      zero this has exactly one solution, so passing it is being equal to `direct`.
  * lookup_columns    the explicit a_j, b_j of the lookup form: k columns 1 / (beta + f_j) and the column -m / (beta + T)
  * multiplicities    by a dict: the least row per table value, the counts at those rows, the row of every looked-up value
  * valid_lookup      lookup columns drawn from a table, with the table's multiplicities: last = 0 for every beta
  * to_limbs / from_limbs   tests/grand_product_oracle.py's
"""
import random

import grand_product_oracle as GO

R = GO.R
to_limbs, from_limbs = GO.to_limbs, GO.from_limbs


def _nums(nums, dens):
    return [[1] * len(dens[0]) for _ in dens] if nums is None else nums


def row_pairs(nums, dens):
    """[(N_i, D_i)]"""
    nums = _nums(nums, dens)
    out = []
    for i in range(len(dens[0])):
        N, D = 0, 1
        for a, b in zip(nums, dens):
            N, D = (N * b[i] + a[i] * D) % R, D * b[i] % R
        out.append((N, D))
    return out


def first_zero(dens):
    """the least row with a zero denominator, or None"""
    for i in range(len(dens[0])):
        if any(b[i] % R == 0 for b in dens):
            return i
    return None


def direct(nums, dens):
    """(phi_0 .. phi_(n-1), phi_n) by the definition; no denominator may be zero"""
    nums = _nums(nums, dens)
    phi, acc = [], 0
    for i in range(len(dens[0])):
        phi.append(acc)
        for a, b in zip(nums, dens):
            acc = (acc + a[i] * pow(b[i], R - 2, R)) % R
    return phi, acc


def check(nums, dens, phi, last):
    """is (phi, last) the running sum of the columns?  No inversion; no denominator may be zero"""
    pairs = row_pairs(nums, dens)
    n = len(pairs)
    if len(phi) != n or n == 0 or phi[0] != 0 or any(D == 0 for _, D in pairs):
        return False
    nxt = list(phi[1:]) + [last]
    return all(((pn - pi) * D - N) % R == 0 for pi, pn, (N, D) in zip(phi, nxt, pairs))


def lookup_columns(lookups, table, mult, beta):
    """(a columns, b columns) of the lookup form: k + 1 of each"""
    n = len(table)
    a = [[1] * n for _ in lookups] + [[(R - m) % R for m in mult]]
    b = [[(beta + f) % R for f in col] for col in lookups] + [[(beta + t) % R for t in table]]
    return a, b


def multiplicities(table, lookups):
    """(counts per table row, rows per lookup column, the least row i of the lookup columns holding a value in no table row or
    None).  A count sits at the LEAST row holding the value; rows[j][i] is that row, or None for a missing value."""
    least = {}
    for r, v in enumerate(table):
        least.setdefault(v, r)
    counts = [0] * len(table)
    rows, missing = [], None
    for col in lookups:
        out = []
        for i, v in enumerate(col):
            r = least.get(v)
            out.append(r)
            if r is None:
                missing = i if missing is None else min(missing, i)
            else:
                counts[r] += 1
        rows.append(out)
    return counts, rows, missing


def valid_lookup(n, k, seed, distinct=None):
    """(lookups, table, mult): a table of n rows over `distinct` different values (default: about n / 2, so that values repeat),
    k lookup columns drawn from it, and the multiplicities of `multiplicities`"""
    rnd = random.Random(seed)
    distinct = max(1, n // 2) if distinct is None else distinct
    pool = [rnd.randrange(R) for _ in range(distinct)]
    table = [pool[rnd.randrange(distinct)] for _ in range(n)]
    lookups = [[table[rnd.randrange(n)] for _ in range(n)] for _ in range(k)]
    counts, _, missing = multiplicities(table, lookups)
    assert missing is None
    return lookups, table, counts
