"""Big-integer restatement of the openings at several point sets (kzg_open_sets and friends):

    polynomial i is opened on the set S_g, g = set_of[i];   F_g = sum_{i in set g} gamma^i P_i;   R_g its interpolant on S_g;
    h = sum_g (F_g - R_g) / Z_(S_g),   proof = [h(s)]G,
    the verifier's sides  A_g = sum_{i in g} gamma^i C_i - [R_g(s)]G,  B_g = Z_(T \\ S_g)(s),  B_T = Z_T(s),  T the union of the sets.

h is computed by explicit long division of every F_g by its vanishing polynomial (open_points_oracle.poly_div_vanishing), NOT by
the regrouping by point the device uses.  Polynomials are lists of Python integers mod r, all of one length; everything is
linear in the coefficients, so the same functions serve plain values and blst_fr images (open_combined_oracle), and only a
scalar of a group element takes the factor 2^256 out."""
import open_combined_oracle as CO
import open_points_oracle as PO
import trapdoor_oracle as TO

R = TO.R
RINV = CO.RINV
# a primitive 8th root of unity: 7^((r - 1) / 8), 7 the generator the library's domains use
ROOT8 = pow(7, (R - 1) // 8, R)

# the five shapes of the tests, as (t, set_of, the sets as lists of indices into a list of sixteen distinct points)
SHAPES = {
    "one_point": (3, [0, 0, 0], [[0]]),
    "sixteen_points": (1, [0], [list(range(16))]),
    "plonk": (10, [0, 1, 0, 0, 1, 0, 0, 0, 1, 0], [[0], [1]]),  # {z}, {z w}; set_of interleaved, not sorted
    "overlapping": (5, [1, 0, 2, 1, 0], [[0], [1, 0, 2], [3, 2]]),  # S0 = {a}, S1 = {b, a, c}, S2 = {d, c}
    "eight_pairs": (10, [3, 0, 7, 1, 6, 2, 5, 4, 0, 3], [[2 * g, 2 * g + 1] for g in range(8)]),
}


def shape(name, points):
    """(t, set_of, sets) with the sets as lists of field elements; points: sixteen distinct ones"""
    t, set_of, index_sets = SHAPES[name]
    return t, list(set_of), [[points[j] % R for j in s] for s in index_sets]


def distinct_points(sets):
    """T: the distinct points over all sets, in order of first appearance"""
    out = []
    for s in sets:
        for z in s:
            if z % R not in out:
                out.append(z % R)
    return out


def set_polynomial(polys, set_of, g, gamma):
    """F_g (no truncation)"""
    n = len(polys[0])
    gs = CO.powers(gamma % R, len(polys))
    members = [i for i in range(len(polys)) if set_of[i] == g]
    return [sum(gs[i] * polys[i][j] for i in members) % R for j in range(n)]


def values(polys, set_of, sets):
    """ys[i]: the values of polynomial i on its set, in the set's point order"""
    return [[TO.poly_eval(p, z % R) for z in sets[g]] for p, g in zip(polys, set_of)]


def quotient(polys, set_of, sets, gamma):
    """h without trailing zeros: the sum over the sets of the explicit quotients of F_g by Z_(S_g)"""
    h = []
    for g, s in enumerate(sets):
        q, _ = PO.poly_div_vanishing(set_polynomial(polys, set_of, g, gamma), [z % R for z in s])
        if len(q) > len(h):
            h += [0] * (len(q) - len(h))
        for j, c in enumerate(q):
            h[j] = (h[j] + c) % R
    return CO.truncate(h)


def proof_scalar(polys, set_of, sets, gamma, s):
    """h(s) = sum_g (F_g(s) - R_g(s)) / Z_(S_g)(s), from the secret of the setup: no division of polynomials, no MSM"""
    return sum(TO.multiproof_scalar(set_polynomial(polys, set_of, g, gamma), [z % R for z in sets[g]], s)
               for g in range(len(sets))) % R


def interpolant_eval(zs, vs, x):
    """the interpolant of (z_j, v_j) at x, Lagrange form"""
    acc = 0
    for i, (zi, vi) in enumerate(zip(zs, vs)):
        num, den = 1, 1
        for j, zj in enumerate(zs):
            if j != i:
                num, den = num * (x - zj) % R, den * (zi - zj) % R
        acc = (acc + vi * num * pow(den, R - 2, R)) % R
    return acc


def vanishing_eval(zs, x):
    acc = 1
    for z in zs:
        acc = acc * (x - z) % R
    return acc


def verifier_sides(commitment_scalars, set_of, sets, ys, gamma, s):
    """([(a_g, b_g)], b_T) as scalars of G1 and G2: the check is sum_g a_g b_g == w b_T for the proof [w]G"""
    t = len(commitment_scalars)
    gs = CO.powers(gamma % R, t)
    T = distinct_points(sets)
    pairs = []
    for g, zs in enumerate(sets):
        zs = [z % R for z in zs]
        members = [i for i in range(t) if set_of[i] == g]
        c = sum(gs[i] * commitment_scalars[i] for i in members) % R
        vs = [sum(gs[i] * ys[i][j] for i in members) % R for j in range(len(zs))]
        rest = [z for z in T if z not in zs]
        pairs.append(((c - interpolant_eval(zs, vs, s)) % R, vanishing_eval(rest, s)))
    return pairs, vanishing_eval(T, s)
