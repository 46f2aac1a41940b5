"""Big-integer restatement of the multilinear openings (kzg_ml_fold .. kzg_ml_verify; Gemini / HyperKZG).

    n = 2^l values f, variable x_i = bit i of the index:   f~(u) = sum_j f[j] prod_i (bit_i(j) ? u_i : 1 - u_i)
    folds   f_(i+1)[j] = f_i[2j] + u_i (f_i[2j+1] - f_i[2j]),  f_0 = f,  f_l = [v]
    values  y_(i,0) = f_i(r), y_(i,1) = f_i(-r), y_(i,2) = f_i(r^2)  (f_i read as coefficients)
    F = sum_{i<l} gamma^i f_i,   W = [(F - I) / Z (s)]G  over the points r, -r, r^2
    (*)  2 r f_(i+1)(r^2) = r (1 - u_i) (y_(i,0) + y_(i,1)) + u_i (y_(i,0) - y_(i,1)),  f_l(r^2) := v

Everything is linear in the values, so the same functions serve plain integers and blst_fr images; u, r, gamma are plain."""
import numpy as np

import open_combined_oracle as CO
import trapdoor_oracle as TO

R = TO.R
RINV = CO.RINV
HALF_UP = (R + 1) // 2  # 1 / 2
SPECIAL_US = (0, 1, R - 1, HALF_UP)


def hypercube_eval(f, u):
    """f~(u) by the definition: 2^l products of l factors"""
    ell = len(u)
    assert len(f) == 1 << ell
    acc = 0
    for j, c in enumerate(f):
        w = c
        for i in range(ell):
            w = w * (u[i] if (j >> i) & 1 else 1 - u[i]) % R
        acc = (acc + w) % R
    return acc


def folds(f, u):
    """[f_1, .., f_l]"""
    out, cur = [], [c % R for c in f]
    for ui in u:
        cur = [(cur[2 * j] + ui * (cur[2 * j + 1] - cur[2 * j])) % R for j in range(len(cur) // 2)]
        out.append(cur)
    return out


def pyramid(f, u):
    """the n - 1 values of f_1 .. f_l packed: level i at offset n - (n >> (i - 1))"""
    return [c for level in folds(f, u) for c in level]


def level_offset(n, i):
    return n - (n >> (i - 1))


def points(r):
    return [r % R, -r % R, r * r % R]


def values(f, u, r):
    """ys[i] = [f_i(r), f_i(-r), f_i(r^2)] for i < l"""
    levels = [[c % R for c in f]] + folds(f, u)[:-1]
    return [[TO.poly_eval(p, z) for z in points(r)] for p in levels]


def padded_stack(f, u):
    """[f_0 | f_1 | .. | f_(l-1)], each padded with zeros to n"""
    n = len(f)
    levels = [[c % R for c in f]] + folds(f, u)[:-1]
    return [p + [0] * (n - len(p)) for p in levels]


def combined(f, u, gamma):
    """F = sum_i gamma^i f_i"""
    stack = padded_stack(f, u)
    gs = CO.powers(gamma % R, len(stack))
    return [sum(g * p[j] for g, p in zip(gs, stack)) % R for j in range(len(f))]


def proof_scalar(f, u, r, gamma, s):
    """the scalar of W from the secret of the setup (f plain values)"""
    return TO.multiproof_scalar(combined(f, u, gamma), points(r), s)


def fold_commitment_scalars(f, u, s):
    """the scalars of C_1 .. C_(l-1)"""
    return [TO.commitment_scalar(p, s) for p in folds(f, u)[:-1]]


def star_holds(u, v, ys, r):
    """the verifier's relation for every level"""
    ell = len(u)
    for i in range(ell):
        nxt = ys[i + 1][2] if i + 1 < ell else v
        lhs = 2 * r * nxt % R
        rhs = (r * (1 - u[i]) * (ys[i][0] + ys[i][1]) + u[i] * (ys[i][0] - ys[i][1])) % R
        if lhs != rhs:
            return False
    return True


# ---- input families -----------------------------------------------------------------------------------------------------------
def random_images(n, seed):
    """(n, 4) uint64 canonical images"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, R >> 192, size=n, dtype=np.uint64)
    return a


def family(kind, n, seed=0):
    """(n, 4) uint64 images: random, all r - 1, equal pairs, or a single non-zero value at the index the name gives"""
    if kind == "random":
        return random_images(n, seed)
    if kind == "max":
        return np.tile(CO.limbs_from_images([R - 1]), (n, 1))
    if kind == "pairs":  # f[2j+1] = f[2j]: the first fold gives the evens whatever u_0 is
        a = random_images(n, seed)
        a[1::2] = a[0::2]
        return a
    assert kind.startswith("single")
    at = {"single0": 0, "single_last": n - 1, "single2047": min(2047, n - 1), "single2048": 2048 % n}[kind]
    a = np.zeros((n, 4), dtype=np.uint64)
    a[at] = random_images(1, seed + 1)[0] | np.uint64(1)
    return a


FAMILIES = ("random", "max", "pairs", "single0", "single_last", "single2047", "single2048")


def random_scalar(seed):
    return int(np.random.default_rng(seed).integers(1, 1 << 62)) * 0x9E3779B97F4A7C15F39CC0605CEDC835 % R


def point_u(ell, kind, seed=0):
    """u: random, or the special values 0, 1, r - 1, 1/2 rotated by `kind` so that every level meets each of them over four kinds
    (levels 10 and 11, the tile boundary, included)"""
    if kind == "random":
        return [random_scalar(seed * 64 + i + 1) for i in range(ell)]
    return [SPECIAL_US[(i + kind) % 4] for i in range(ell)]
