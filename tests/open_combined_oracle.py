"""Big-integer restatement of the combined openings (kzg_open_combined and friends):

    F = sum_i gamma^i P_i,   y_i = P_i(z),   q = (F - F(z)) / (X - z),   proof = [q(s)]G,
    the verifier's claim  C = sum_i gamma^i C_i,  y = sum_i gamma^i y_i.

Polynomials are lists of Python integers mod r, all of one length.  Everything here is linear in the coefficients, so the
same functions serve plain values and blst_fr images (value * 2^256 mod r, what the C-ABI carries): F, the y_i and q of
images are the images of F, the y_i and q.  Only where an integer becomes a scalar of a group element (proof, with
images=True) is the factor 2^256 taken out.  The proof is [v]G for the scalar v that tests/trapdoor_oracle.py gives for
F, with the secret of the setup known: no MSM."""
import numpy as np

import trapdoor_oracle as TO

R = TO.R
RINV = pow(1 << 256, -1, R)
INFINITY = bytes([0xC0]) + bytes(47)  # the compressed point at infinity


def powers(gamma, t):
    out, g = [], 1
    for _ in range(t):
        out.append(g)
        g = g * gamma % R
    return out


def combine(polys, gamma):
    """the n coefficients of F (no truncation)"""
    gs = powers(gamma % R, len(polys))
    if len(polys) == 1:
        return [c % R for c in polys[0]]
    return [sum(g * p[j] for g, p in zip(gs, polys)) % R for j in range(len(polys[0]))]


def values(polys, z):
    return [TO.poly_eval(p, z % R) for p in polys]


def truncate(f):
    """the reference's truncation: trailing zero coefficients dropped"""
    n = len(f)
    while n and f[n - 1] % R == 0:
        n -= 1
    return f[:n]


def quotient(f, z):
    """(q, F(z)) for q = (F - F(z)) / (X - z) of the truncated F; q is empty when F is constant or zero"""
    f = truncate(f)
    q = [0] * max(len(f) - 1, 0)
    acc = 0
    for i in range(len(f) - 1, 0, -1):
        acc = (acc * z + f[i]) % R
        q[i - 1] = acc
    return q, ((acc * z + f[0]) % R if f else 0)


def proof_scalar(f, z, s):
    """q(s) for the truncated F, None where the proof is infinity by rule (n' <= 1)"""
    f = truncate(f)
    if len(f) <= 1:
        return None
    return TO.proof_scalar(f, z, s)


def proof(oracle, f, z, s, images=False):
    """the compressed proof of F at z; images: F is given as blst_fr images"""
    v = proof_scalar(f, z, s)
    if v is None:
        return INFINITY
    return TO.g1_scalar(oracle, v * RINV % R if images else v)


def combined_claim(commitment_scalars, ys, gamma):
    """(c, y) with C = [c]G for commitments C_i = [c_i]G"""
    gs = powers(gamma % R, len(ys))
    return sum(g * c for g, c in zip(gs, commitment_scalars)) % R, sum(g * y for g, y in zip(gs, ys)) % R


def images_from_limbs(arr):
    """(n, 4) uint64 -> the n 256-bit integers the rows hold"""
    b = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def limbs_from_images(vals):
    b = b"".join(int(v).to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype="<u8").reshape(-1, 4).astype(np.uint64)
