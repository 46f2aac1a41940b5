"""Big-integer reference for kzg_recover_cells_and_proofs: the coset erasure decode of DESIGN.md section 4.9 in Python
integers mod r, on top of ntt_oracle and cells_oracle.

Domain of N = 2^K points, cells of l = 2^t, M = N / l cells; cell j is {w_N^(j + M i) : i < l} (cells_oracle.cells order).
S = the missing cells, Z'(Y) = prod_{j in S} (Y - w_M^j), Z(X) = Z'(X^l).  With g = 7:
    D[j + M i] = E_j[i] Z'(w_M^j) (received j), 0 (missing);  PZ = INTT(D);  PZ_i g^i;  NTT;  / Z'(g^l w_M^(e mod M));
    INTT;  P_i g^-i.
P is accepted when its coefficients at [n, N) are all zero.
"""
import cells_oracle as CO
import ntt_oracle as NO

R = NO.R
G = NO.GENERATOR


def missing_cells(K, t, ids):
    got = set(ids)
    return [j for j in range((1 << K) >> t) if j not in got]


def vanishing_prime(K, t, missing):
    """Z'(Y) = prod_{j in missing} (Y - w_M^j), coefficients low to high"""
    wm = NO.domain_root(K - t)
    return CO.vanishing([pow(wm, j, R) for j in missing])


def vanishing_full(K, t, missing):
    """Z(X) = Z'(X^l) as coefficients: Z' spread out by l"""
    l = 1 << t
    zp = vanishing_prime(K, t, missing)
    z = [0] * ((len(zp) - 1) * l + 1)
    for i, c in enumerate(zp):
        z[i * l] = c
    return z


def decode(n, K, t, ids, received):
    """received[s] = the l values of cell ids[s] (one polynomial).  Returns (coefficients [0, n), ok): ok is False when the
    decoded coefficients at [n, N) are not all zero"""
    N, l = 1 << K, 1 << t
    M = N >> t
    missing = missing_cells(K, t, ids)
    zp = vanishing_prime(K, t, missing)
    wm = NO.domain_root(K - t)
    d = [0] * N
    for j, vals in zip(ids, received):
        zj = CO.poly_eval(zp, pow(wm, j, R))
        for i, v in enumerate(vals):
            d[j + M * i] = v * zj % R
    pz = NO.intt(d)
    gi = 1
    for i in range(N):
        pz[i] = pz[i] * gi % R
        gi = gi * G % R
    ev = NO.ntt(pz)
    gl = pow(G, l, R)
    inv = NO.batch_inverse([CO.poly_eval(zp, gl * pow(wm, e, R) % R) for e in range(M)])
    q = NO.intt([v * inv[e % M] % R for e, v in enumerate(ev)])
    ginv = pow(G, R - 2, R)
    gi = 1
    for i in range(N):
        q[i] = q[i] * gi % R
        gi = gi * ginv % R
    return q[:n], not any(q[n:])


def lagrange(xs, ys):
    """coefficients of the polynomial of degree < len(xs) through the points (xs distinct)"""
    v = CO.vanishing(xs)
    out = [0] * len(xs)
    for x, y in zip(xs, ys):
        # v / (X - x) by synthetic division, then weight y / prod_{x' != x} (x - x')
        q = [0] * len(xs)
        acc = 0
        for i in range(len(v) - 1, 0, -1):
            acc = (v[i] + acc * x) % R
            q[i - 1] = acc
        w = y * pow(CO.poly_eval(q, x), R - 2, R) % R
        for i in range(len(xs)):
            out[i] = (out[i] + w * q[i]) % R
    return out
