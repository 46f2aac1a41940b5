"""Big-integer restatement of kzg_evaluate_evaluations_batch and kzg_verify_openings_batch / _lincomb (DESIGN.md section
4.11), independent of the library: the barycentric value of a polynomial held in evaluation form (and the in-domain case),
and the two G1 sides of the random-linear-combination check for given weights, over any group given as (add, mul, zero) --
G1 points of oracle/bigint_twin.py for the byte-for-byte comparison, or plain scalars mod r (discrete logarithms to G,
through the trapdoor of tests/trapdoor_oracle.py) so that both sides are [v]G for a v computed in O(k)."""
import bigint_twin as T
import ntt_oracle as NO
import trapdoor_oracle as TO

R = NO.R


def barycentric(evals, z):
    """P(z) for the P of degree < n = len(evals) with P(w^i) = evals[i]:
    (z^n - 1) / n sum_i f_i w^i / (z - w^i), and f_j itself where z = w^j.  Written out here (one inversion per term) rather
    than taken from ntt_oracle, which the tests compare it with through the interpolated coefficients."""
    n = len(evals)
    w = NO.domain_root(NO.log2_exact(n))
    z %= R
    acc, x = 0, 1
    for f in evals:
        if x == z:
            return f % R
        acc = (acc + f * x % R * pow(z - x, R - 2, R)) % R
        x = x * w % R
    return (pow(z, n, R) - 1) * pow(n, R - 2, R) % R * acc % R


def sides(commitments, idx, zs, ys, proofs, weights, g, add, mul, zero):
    """(LHS, RHS) = (sum_t rho_t pi_t, sum_b U_b C_b - [sum_t rho_t y_t] g + sum_z [z] T_z), T_z = sum_{t: z_t = z} rho_t pi_t"""
    lhs = zero
    U = [0] * len(commitments)
    Tz = {}
    sy = 0
    for b, z, y, pi, w in zip(idx, zs, ys, proofs, weights):
        term = mul(pi, w % R)
        lhs = add(lhs, term)
        U[b] = (U[b] + w) % R
        Tz[z % R] = add(Tz.get(z % R, zero), term)
        sy = (sy + w * y) % R
    rhs = zero
    for C, u in zip(commitments, U):
        rhs = add(rhs, mul(C, u))
    rhs = add(rhs, mul(g, -sy % R))
    for z, Tv in Tz.items():
        rhs = add(rhs, mul(Tv, z))
    return lhs, rhs


def scalar_sides(commitments, idx, zs, ys, proofs, weights):
    """the same over discrete logarithms: commitments P_b(s), proofs q_t(s), G -> 1"""
    return sides(commitments, idx, zs, ys, proofs, weights, 1, lambda a, b: (a + b) % R, lambda p, k: p * k % R, 0)


def g1_sides(commitments, idx, zs, ys, proofs, weights):
    """the same over G1 points of the twin (None = infinity)"""
    return sides(commitments, idx, zs, ys, proofs, weights, T.G1, T.g1_add, lambda p, k: T.g1_mul(p, k % R), T.INF)


def trapdoor_records(polys, idx, zs, s, ys=None):
    """(commitment scalars, proof scalars, values) of the records (polys[idx[t]] at zs[t]) under the secret s"""
    coms = [TO.commitment_scalar(c, s) for c in polys]
    vals = [TO.poly_eval(polys[b], z) for b, z in zip(idx, zs)] if ys is None else list(ys)
    prfs = [TO.proof_scalar(polys[b], z, s) for b, z in zip(idx, zs)]
    return coms, prfs, vals


def holds(commitments, idx, zs, ys, proofs, weights, s):
    """the pairing equation e(LHS, [s]G2) == e(RHS, G2) over discrete logarithms: s LHS == RHS"""
    lhs, rhs = scalar_sides(commitments, idx, zs, ys, proofs, weights)
    return s % R * lhs % R == rhs
