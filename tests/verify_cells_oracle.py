"""Big-integer restatement of kzg_verify_cells_batch / kzg_verify_cells_lincomb: the two G1 sides
of the random-linear-combination check for given weights, over any group given as (add, mul, zero) -- G1 points of
oracle/bigint_twin.py for the byte-for-byte comparison, or plain scalars mod r (discrete logarithms to G) for the algebra
with a known secret -- and the G1 subgroup test the device runs."""
import bigint_twin as T
import ntt_oracle as NO

R = NO.R
P = T.P
Z_ABS = 0xD201000000010000  # |z|, z = -0xd201000000010000
LAMBDA = Z_ABS * Z_ABS - 1  # z^2 - 1: [lambda](x, y) = (beta x, y) on G1, r = lambda^2 + lambda + 1
# beta of fk20_kernels.hip's fq_beta(): its balanced radix-2^30 digits are beta * 2^390 mod p
_BETA_DIGITS = [0x1c907181, -0x3421b7a, -0x19a8b3c1, -0xcdb8a13, 0x1c3ebc1c, -0x611979c, 0x16ffa857, -0x13cb6601, 0x550bd17,
                0x14cbac30, 0x17d18c86, -0x1ea6a609, 0x9c6d5]
BETA = sum(d << (30 * i) for i, d in enumerate(_BETA_DIGITS)) * pow(2, -390, P) % P
BETA2 = BETA * BETA % P  # = p - 1 - beta: (beta^2 x, y) = [-z^2](x, y) on G1


def g1_in_subgroup(pt):
    """Scott's test (ePrint 2021/1130): P in G1 iff [z^2] P == (beta^2 x, -y); infinity passes"""
    if pt is T.INF:
        return True
    x, y = pt
    return T.g1_mul(pt, Z_ABS * Z_ABS) == (BETA2 * x % P, -y % P)


def g1_in_subgroup_by_order(pt):
    return T.g1_mul(pt, R) is T.INF


def glv_weight(a, b):
    """the weight a + b lambda of a record (a, b < 2^64): a field element below 2^193 < r"""
    return (a + b * LAMBDA) % R


def interpolant(K, t, j, vals):
    """coefficients of I (degree < l) with I(w_N^(j + M i)) = vals[i]: c_i = h_j^-i / l sum_k vals[k] w_l^(-i k)"""
    l = 1 << t
    wl_inv = pow(NO.domain_root(t), -1, R)
    h_inv = pow(NO.domain_root(K), -j % (1 << K), R) if K else 1
    l_inv = pow(l, -1, R)
    out = []
    for i in range(l):
        y = sum(v * pow(wl_inv, i * k, R) for k, v in enumerate(vals)) % R
        out.append(y * pow(h_inv, i, R) * l_inv % R)
    return out


def combined_interpolant(K, t, ids, values, weights):
    """A = sum_t rho_t I_t, l coefficients"""
    A = [0] * (1 << t)
    for j, vals, w in zip(ids, values, weights):
        for i, c in enumerate(interpolant(K, t, j, vals)):
            A[i] = (A[i] + w * c) % R
    return A


def sides(K, t, commitments, idx, ids, values, proofs, weights, srs, add, mul, zero):
    """(LHS, RHS) = (sum_t rho_t pi_t, sum_b U_b C_b - [A(s)] + sum_j [a_j] T_j); srs: [s^i]G1 for i < l in the group"""
    M = (1 << K) >> t
    lhs = zero
    U = [0] * len(commitments)
    Tj = {}
    for b, j, pi, w in zip(idx, ids, proofs, weights):
        term = mul(pi, w)
        lhs = add(lhs, term)
        U[b] = (U[b] + w) % R
        Tj[j] = add(Tj.get(j, zero), term)
    rhs = zero
    for C, u in zip(commitments, U):
        rhs = add(rhs, mul(C, u))
    for i, a in enumerate(combined_interpolant(K, t, ids, values, weights)):
        rhs = add(rhs, mul(srs[i], -a % R))
    aM = NO.domain_root(K - t) if M > 1 else 1
    for j, Tv in Tj.items():
        rhs = add(rhs, mul(Tv, pow(aM, j, R)))
    return lhs, rhs


def scalar_sides(K, t, commitments, idx, ids, values, proofs, weights, s):
    """the same over discrete logarithms: commitments P_b(s), proofs q_t(s), [s^i]G1 -> s^i"""
    l = 1 << t
    return sides(K, t, commitments, idx, ids, values, proofs, weights, [pow(s, i, R) for i in range(l)],
                 lambda a, b: (a + b) % R, lambda p, k: p * k % R, 0)


def g1_sides(K, t, commitments, idx, ids, values, proofs, weights, srs):
    """the same over G1 points of the twin (None = infinity)"""
    return sides(K, t, commitments, idx, ids, values, proofs, weights, srs, T.g1_add, lambda p, k: T.g1_mul(p, k % R), T.INF)
