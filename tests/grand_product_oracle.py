"""Independent references for the grand-product entry points (kzg_grand_product, kzg_permutation_product,
kzg_permutation_commit), in Python integers mod r.

t numerator columns a_j and t denominator columns b_j of n values each (lists of t lists); A_i = prod_j a_j[i], B_i likewise.
  * direct            z_0 = 1, z_(i+1) = z_i A_i / B_i with one modular inverse per step: the definition, for small n
  * check             no inversion at all: z_0 = 1, z_(i+1) B_i = z_i A_i for every i, and last B_(n-1) = z_(n-1) A_(n-1).
                      With no B_i zero this has exactly one solution, so passing it is being equal to `direct`.
  * perm_columns      the a_j, b_j of the permutation form: a_j[i] = f_j[i] + beta k_j w^i + gamma,
                      b_j[i] = f_j[i] + beta sigma_j[i] + gamma over the domain of w = ntt_oracle.domain_root(k)
  * true_permutation  a random permutation of the t n cell labels k_j w^i with wires constant on its cycles: last = 1
  * to_limbs / from_limbs   plain values <-> the (n, 4) uint64 array of blst_fr images, through bytes (fast at 2^18 values)
"""
import random

import numpy as np

import ntt_oracle as NO

R = NO.R
R256 = pow(2, 256, R)
R256_INV = pow(R256, -1, R)
GENERATOR = 7  # the multiplicative generator the domain roots are powers of: 7^j lies in no proper subgroup for small j > 0


def to_limbs(values):
    return np.frombuffer(b"".join((v % R * R256 % R).to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(-1, 4).copy()


def from_limbs(arr):
    raw = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") * R256_INV % R for i in range(0, len(raw), 32)]


def products(cols):
    """[prod_j cols[j][i] for i]"""
    out = list(cols[0])
    for c in cols[1:]:
        out = [x * y % R for x, y in zip(out, c)]
    return out


def first_zero(dens):
    """the least i with B_i = 0, or None"""
    for i, b in enumerate(products(dens)):
        if b == 0:
            return i
    return None


def direct(nums, dens):
    """(z_0 .. z_(n-1), z_n) by the definition; no B_i may be zero"""
    z, acc = [], 1
    for a, b in zip(products(nums), products(dens)):
        z.append(acc)
        acc = acc * a % R * pow(b, R - 2, R) % R
    return z, acc


def check(nums, dens, z, last):
    """is (z, last) the grand product of the columns?  No inversion; no B_i may be zero"""
    A, B = products(nums), products(dens)
    n = len(A)
    if len(z) != n or n == 0 or z[0] != 1 or any(b == 0 for b in B):
        return False
    nxt = list(z[1:]) + [last]
    return all((zn * b - zi * a) % R == 0 for zi, zn, a, b in zip(z, nxt, A, B))


def shifts(t):
    """t coset shifts: 1, 7, 49, ... (distinct cosets of every power-of-two domain)"""
    return [pow(GENERATOR, j, R) for j in range(t)]


def domain(k):
    w = NO.domain_root(k)
    pts = [1] * (1 << k)
    for i in range(1, len(pts)):
        pts[i] = pts[i - 1] * w % R
    return pts


def perm_columns(wires, sigmas, ks, beta, gamma):
    """(a columns, b columns) of the permutation form"""
    n = len(wires[0])
    pts = domain(NO.log2_exact(n))
    a = [[(f + beta * k % R * p + gamma) % R for f, p in zip(col, pts)] for col, k in zip(wires, ks)]
    b = [[(f + beta * s + gamma) % R for f, s in zip(col, sig)] for col, sig in zip(wires, sigmas)]
    return a, b


def identity_sigmas(k, ks):
    """the permutation that moves nothing: sigma_j[i] = k_j w^i"""
    pts = domain(k)
    return [[kj * p % R for p in pts] for kj in ks]


def true_permutation(k, t, ks, seed):
    """(wires, sigmas): a random permutation of the t n cells, sigma_j[i] the label of the image of cell (j, i), and wire values
    constant on its cycles"""
    rnd = random.Random(seed)
    n = 1 << k
    pts = domain(k)
    cells = [(j, i) for j in range(t) for i in range(n)]
    image = list(range(len(cells)))
    rnd.shuffle(image)
    wires = [[None] * n for _ in range(t)]
    sigmas = [[0] * n for _ in range(t)]
    for c, (j, i) in enumerate(cells):
        jj, ii = cells[image[c]]
        sigmas[j][i] = ks[jj] * pts[ii] % R
        if wires[j][i] is None:  # a new cycle: one value all along it
            v = rnd.randrange(R)
            d = c
            while True:
                dj, di = cells[d]
                if wires[dj][di] is not None:
                    break
                wires[dj][di] = v
                d = image[d]
    return wires, sigmas
