"""Reference computations for the multiproof tests (tests/test_open_points*.py), built only from what the C oracle and the
twins under oracle/ already provide -- the quotient is computed the OTHER way than the library:

  * quotient_points / open_points: k chained synthetic divisions by (X - z_i) with the oracle's single-root division
    (oracle_quotient, its remainder passed as the claim so it never refuses), i.e. the quotient of P by Z = prod (X - z_i);
    P = q Z + I makes it (P - I) / Z.  The claims are checked first with oracle_poly_evaluate, the proof is committed by
    the oracle's Pippenger.
  * poly_div_vanishing: schoolbook long division by Z in Python big ints (bigint_twin's field).
  * verify_points: the pairing check with Z(s) and I(s) computed as scalars from the known secret (pairing_twin), independent
    of the library's G2 code."""
import numpy as np

import bigint_twin as T
import pairing_twin as PT

R = T.R
OK, ERR_DEGREE_TOO_HIGH, ERR_REMAINDER = 0, -1, -3  # the oracle's codes (kzg_oracle.h), which mirror the library's


def quotient_points(oracle, coeffs, zs, ys):
    """(rc, q) for P = coeffs at the points zs with claims ys (k x 4 Montgomery limbs each); q has n' - k rows or none"""
    c = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
    zs = np.ascontiguousarray(zs, dtype=np.uint64).reshape(-1, 4)
    ys = np.ascontiguousarray(ys, dtype=np.uint64).reshape(-1, 4)
    for z, y in zip(zs, ys):
        if not np.array_equal(oracle.poly_evaluate(c, z), y):
            return ERR_REMAINDER, np.zeros((0, 4), np.uint64)
    cur = c
    for z in zs:
        if len(cur) == 0:
            break
        rc, cur = oracle.quotient(cur, z, oracle.poly_evaluate(cur, z))
        assert rc == OK
    return OK, np.ascontiguousarray(cur, dtype=np.uint64).reshape(-1, 4)


def open_points(oracle, coeffs, zs, ys, srs, threads=8):
    """(rc, proof) as blst_p1 limbs; q longer than the SRS -> ERR_DEGREE_TOO_HIGH, q = 0 -> infinity (all zero)"""
    rc, q = quotient_points(oracle, coeffs, zs, ys)
    if rc != OK:
        return rc, None
    if len(q) > srs.nbytes // 144:
        return ERR_DEGREE_TOO_HIGH, None
    if len(q) == 0:
        return OK, np.zeros(18, dtype=np.uint64)
    return oracle.commit_pippenger(q, srs, threads)


def poly_div_vanishing(coeffs, zs):
    """(q, rem) with P = q * Z + rem, Z = prod (X - z_i), integers mod r.  rem is the interpolant of (z_i, P(z_i))."""
    zc = [1]
    for z in zs:  # multiply by (X - z)
        zc = [((zc[j - 1] if j else 0) - z * (zc[j] if j < len(zc) else 0)) % R for j in range(len(zc) + 1)]
    p = [x % R for x in coeffs]
    while p and p[-1] == 0:
        p.pop()
    k = len(zs)
    if len(p) <= k:
        return [], p
    q = [0] * (len(p) - k)
    for d in range(len(p) - 1, k - 1, -1):  # Z is monic: the leading term goes straight into q
        t = p[d]
        q[d - k] = t
        for j in range(k + 1):
            p[d - k + j] = (p[d - k + j] - t * zc[j]) % R
    rem = p[:k]
    while rem and rem[-1] == 0:
        rem.pop()
    return q, rem


def verify_points(commitment, proof, zs, ys, secret_be):
    """e(proof, [Z(s)]G2) == e(commitment - [I(s)]G1, G2) with Z(s), I(s) (Lagrange form) from the known secret;
    commitment, proof: twin affine points"""
    s = T.fr_from_be_bytes(secret_be)
    zs = [z % R for z in zs]
    zv, iv = 1, 0
    for z in zs:
        zv = zv * (s - z) % R
    for i, (zi, yi) in enumerate(zip(zs, ys)):
        num, den = 1, 1
        for j, zj in enumerate(zs):
            if j != i:
                num, den = num * (s - zj) % R, den * (zi - zj) % R
        iv = (iv + yi * num * pow(den, R - 2, R)) % R
    rhs = T.g1_add(commitment, T.g1_neg(T.g1_mul(T.G1, iv)))
    return PT.pairing_product_is_one([(proof, PT.g2_mul(PT.G2, zv)), (T.g1_neg(rhs), PT.G2)])
