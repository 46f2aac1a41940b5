"""Independent references for the quotient of a permutation argument (kzg_coset_extend, kzg_permutation_constraints_coset,
kzg_vanishing_quotient, kzg_permutation_quotient), in Python integers mod r, on top of ntt_oracle and
grand_product_oracle.

n = 2^k, H = <w_n>, N = e n, coset points x_i = 7 w_N^i in natural order.
  * coset_points / coset_extend_direct   the definition: Horner at every x_i (small sizes)
  * coset_extend                          the same values through ntt_oracle's transform of the twisted, padded coefficients
  * z_of                                  the accumulator z_0 .. z_(n-1) of a permutation argument and z_n (grand_product_oracle)
  * num_coeffs                            Num as a coefficient vector, by polynomial arithmetic over a SUBGROUP large enough for its
                                          degree (products of values, one inverse transform) -- no coset, no division
  * divide_vanishing                      exact division by X^n - 1 from the top coefficient down: (quotient, remainder)
  * constraints_on_coset                  Num(x_i) / Z_H(x_i) point by point from any N-value columns (one modular inverse per point)
  * check_at                              no inversion at all: T(zeta) (zeta^n - 1) == Num(zeta), every polynomial by Horner
"""
import grand_product_oracle as GO
import ntt_oracle as NO

R = NO.R
G = 7


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def coset_points(log_N):
    w = NO.domain_root(log_N)
    pts = [G % R] * (1 << log_N)
    for i in range(1, len(pts)):
        pts[i] = pts[i - 1] * w % R
    return pts


def coset_extend_direct(coeffs, log_N):
    return [horner(coeffs, x) for x in coset_points(log_N)]


def coset_extend(coeffs, log_N):
    """the values of sum c_j X^j (any number of coefficients up to N) at the coset points"""
    N = 1 << log_N
    assert 1 <= len(coeffs) <= N
    tw, g = [], 1
    for c in coeffs:
        tw.append(c * g % R)
        g = g * G % R
    return NO.ntt(tw + [0] * (N - len(coeffs)))


def z_of(wires, sigmas, ks, beta, gamma):
    """(z_0 .. z_(n-1), z_n)"""
    a, b = GO.perm_columns(wires, sigmas, ks, beta, gamma)
    return GO.direct(a, b)


def _trim(c):
    c = list(c)
    while c and c[-1] == 0:
        c.pop()
    return c


def num_coeffs(wires, sigmas, z, ks, alpha, beta, gamma, gate=None):
    """Num = G + alpha [z prod (f_j + beta k_j X + gamma) - z(wX) prod (f_j + beta sigma_j + gamma)] + alpha^2 (z - 1) L_0 as
    coefficients (trailing zeros trimmed); the columns and z are n values over H, gate a coefficient vector or None"""
    n, t = len(z), len(wires)
    k = NO.log2_exact(n)
    w = NO.domain_root(k)
    M = 1
    while M < (t + 2) * n:
        M *= 2
    pts = GO.domain(NO.log2_exact(M))
    on = lambda coeffs: NO.ntt(list(coeffs) + [0] * (M - len(coeffs)))
    f = [on(NO.intt(c)) for c in wires]
    s = [on(NO.intt(c)) for c in sigmas]
    zc = NO.intt(z)
    zv = on(zc)
    zr = on([c * pow(w, i, R) % R for i, c in enumerate(zc)])  # z(w X)
    l0 = on([pow(n, R - 2, R)] * n)                            # (X^n - 1) / (n (X - 1)) = (1 / n) (1 + X + .. + X^(n-1))
    vals = []
    for i, x in enumerate(pts):
        a, b = zv[i], zr[i]
        for j in range(t):
            a = a * ((f[j][i] + beta * ks[j] % R * x + gamma) % R) % R
            b = b * ((f[j][i] + beta * s[j][i] + gamma) % R) % R
        vals.append((alpha * (a - b) + alpha * alpha % R * (zv[i] - 1) % R * l0[i]) % R)
    num = NO.intt(vals)
    if gate is not None:
        num = [(a + b) % R for a, b in zip(num + [0] * max(0, len(gate) - len(num)), list(gate) + [0] * max(0, len(num) - len(gate)))]
    return _trim(num)


def divide_vanishing(num, n):
    """(T, remainder) with num = T (X^n - 1) + remainder, deg remainder < n"""
    rem = list(num)
    T = [0] * max(0, len(rem) - n)
    for k in range(len(rem) - 1, n - 1, -1):
        T[k - n] = rem[k]
        rem[k - n] = (rem[k - n] + rem[k]) % R
        rem[k] = 0
    return T, _trim(rem[:n])


def quotient(wires, sigmas, z, ks, alpha, beta, gamma, gate=None):
    """T, asserting a zero remainder"""
    T, rem = divide_vanishing(num_coeffs(wires, sigmas, z, ks, alpha, beta, gamma, gate), len(z))
    assert rem == [], "Num is not divisible by X^n - 1"
    return T


def constraints_on_coset(wires_ext, sigmas_ext, z_ext, n, ks, alpha, beta, gamma, gate=None):
    """Num(x_i) / Z_H(x_i) for i < N from N-value columns (which need not be extensions of anything)"""
    N, t = len(z_ext), len(wires_ext)
    e = N // n
    pts = coset_points(NO.log2_exact(N))
    inv_n = pow(n, R - 2, R)
    out = []
    for i, x in enumerate(pts):
        zh = (pow(x, n, R) - 1) % R
        a, b = z_ext[i], z_ext[(i + e) % N]
        for j in range(t):
            a = a * ((wires_ext[j][i] + beta * ks[j] % R * x + gamma) % R) % R
            b = b * ((wires_ext[j][i] + beta * sigmas_ext[j][i] + gamma) % R) % R
        l0 = zh * inv_n % R * pow(x - 1, R - 2, R) % R
        num = ((gate[i] if gate is not None else 0) + alpha * (a - b) + alpha * alpha % R * (z_ext[i] - 1) % R * l0) % R
        out.append(num * pow(zh, R - 2, R) % R)
    return out


def check_at(zeta, T, wire_coeffs, sigma_coeffs, z_coeffs, n, ks, alpha, beta, gamma, gate_coeffs=None):
    """T(zeta) (zeta^n - 1) == Num(zeta), all from coefficients by Horner; no inversion"""
    w = NO.domain_root(NO.log2_exact(n))
    zv, zr = horner(z_coeffs, zeta), horner(z_coeffs, zeta * w % R)
    a, b = zv, zr
    for fc, sc, k in zip(wire_coeffs, sigma_coeffs, ks):
        f = horner(fc, zeta)
        a = a * ((f + beta * k % R * zeta + gamma) % R) % R
        b = b * ((f + beta * horner(sc, zeta) + gamma) % R) % R
    l0 = horner([pow(n, R - 2, R)] * n, zeta)
    num = (alpha * (a - b) + alpha * alpha % R * (zv - 1) % R * l0 + (horner(gate_coeffs, zeta) if gate_coeffs else 0)) % R
    return horner(T, zeta) * (pow(zeta, n, R) - 1) % R == num
