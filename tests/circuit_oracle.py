"""Independent references for the quotient of a circuit with a resident key (kzg_circuit_create, kzg_circuit_quotient; DESIGN.md
section 4.22), in Python integers mod r, on top of perm_quotient_oracle, grand_product_oracle and ntt_oracle.

A circuit over H = <w_n> has t >= 2 wire columns f_j, linear selectors q_j, a multiplication selector q_M, a constant selector q_C
and permutation columns sigma_j with shifts k_j.  With public inputs PI (n values, added as given) and the caller's term G':

    Gate(X) = sum_j q_j f_j + q_M f_0 f_1 + q_C + PI + G'
    Num(X)  = Gate(X) + (the permutation's numerator of perm_quotient_oracle)

  * satisfied        a circuit whose every row holds: wires and sigmas of a true permutation, random q_j and q_M, and
                     q_C[i] = -(sum_j q_j f_j + q_M f_0 f_1 + PI_i)
  * gate_coeffs      the gate as a coefficient vector: products of values over a SUBGROUP of at least 3 n points, one inverse
                     transform -- no coset, no division
  * quotient         perm_quotient_oracle.quotient with gate = gate_coeffs (asserts a zero remainder); remainder: the same division's
                     remainder
  * check_at         T(zeta) (zeta^n - 1) == Num(zeta) with the gate, every polynomial by Horner, no inversion
"""
import random

import grand_product_oracle as GO
import ntt_oracle as NO
import perm_quotient_oracle as PQ

R = PQ.R


class Circuit:
    """columns as lists of n integers; pi is None or n integers"""

    def __init__(self, ks, wires, sigmas, q_lin, q_mul, q_const, pi):
        self.ks, self.wires, self.sigmas, self.q_lin, self.q_mul, self.q_const, self.pi = ks, wires, sigmas, q_lin, q_mul, q_const, pi
        self.n, self.t = len(q_mul), len(wires)

    def key_columns(self):
        """the 2 t + 2 resident columns in the order of the key: q_lin[0..t), q_mul, q_const, sigma[0..t)"""
        return list(self.q_lin) + [self.q_mul, self.q_const] + list(self.sigmas)


def gate_rows(c, wires=None):
    """the gate's value on every row of H (all zero for a satisfied circuit)"""
    f = c.wires if wires is None else wires
    out = []
    for i in range(c.n):
        v = c.q_mul[i] * f[0][i] % R * f[1][i] + c.q_const[i] + (c.pi[i] if c.pi is not None else 0)
        for j in range(c.t):
            v += c.q_lin[j][i] * f[j][i]
        out.append(v % R)
    return out


def satisfied(k, t, seed, with_pi=True):
    assert t >= 2
    n = 1 << k
    ks = GO.shifts(t)
    wires, sigmas = GO.true_permutation(k, t, ks, seed)
    rnd = random.Random(7000 + 31 * seed + t)
    q_lin = [[rnd.randrange(R) for _ in range(n)] for _ in range(t)]
    q_mul = [rnd.randrange(R) for _ in range(n)]
    pi = [rnd.randrange(R) if i % 3 == 0 else 0 for i in range(n)] if with_pi else None
    c = Circuit(ks, wires, sigmas, q_lin, q_mul, [0] * n, pi)
    c.q_const = [(-v) % R for v in gate_rows(c)]
    assert gate_rows(c) == [0] * n
    return c


def gate_coeffs(c, wires=None, extra=None):
    """Gate as coefficients (trailing zeros trimmed); extra: the coefficients of G' or None"""
    f = c.wires if wires is None else wires
    n = c.n
    M = 4
    while M < 3 * n:
        M *= 2
    on = lambda vals: NO.ntt(NO.intt(list(vals)) + [0] * (M - n))
    fv = [on(col) for col in f]
    qv = [on(col) for col in c.q_lin]
    qm, qc = on(c.q_mul), on(c.q_const)
    pv = on(c.pi) if c.pi is not None else [0] * M
    vals = []
    for i in range(M):
        v = qm[i] * fv[0][i] % R * fv[1][i] + qc[i] + pv[i]
        for j in range(c.t):
            v += qv[j][i] * fv[j][i]
        vals.append(v % R)
    g = NO.intt(vals)
    if extra is not None:
        m = max(len(g), len(extra))
        g = [(a + b) % R for a, b in zip(g + [0] * (m - len(g)), list(extra) + [0] * (m - len(extra)))]
    return PQ._trim(g)


def z_of(c, beta, gamma, wires=None):
    return PQ.z_of(c.wires if wires is None else wires, c.sigmas, c.ks, beta, gamma)


def numerator(c, z, alpha, beta, gamma, wires=None, extra=None):
    f = c.wires if wires is None else wires
    return PQ.num_coeffs(f, c.sigmas, z, c.ks, alpha, beta, gamma, gate_coeffs(c, f, extra))


def quotient(c, z, alpha, beta, gamma, wires=None, extra=None):
    """T, asserting a zero remainder"""
    f = c.wires if wires is None else wires
    return PQ.quotient(f, c.sigmas, z, c.ks, alpha, beta, gamma, gate=gate_coeffs(c, f, extra))


def remainder(c, z, alpha, beta, gamma, wires=None, extra=None):
    return PQ.divide_vanishing(numerator(c, z, alpha, beta, gamma, wires, extra), c.n)[1]


def check_at(zeta, T, c, wire_coeffs, z_coeffs, alpha, beta, gamma, extra=None, key_coeffs=None, pi_coeffs=None):
    """T(zeta) (zeta^n - 1) == Num(zeta), the gate included, all by Horner from coefficients; no inversion.  key_coeffs, pi_coeffs:
    the coefficients of key_columns() and of PI where the caller has them already (large n); else by ntt_oracle"""
    h = PQ.horner
    key = [NO.intt(col) for col in c.key_columns()] if key_coeffs is None else key_coeffs
    t = c.t
    f = [h(fc, zeta) for fc in wire_coeffs]
    gate = h(key[t], zeta) * f[0] % R * f[1] + h(key[t + 1], zeta)
    for j in range(t):
        gate += h(key[j], zeta) * f[j]
    if c.pi is not None:
        gate += h(NO.intt(c.pi) if pi_coeffs is None else pi_coeffs, zeta)
    if extra is not None:
        gate += h(extra, zeta)
    w = NO.domain_root(NO.log2_exact(c.n))
    zv, zr = h(z_coeffs, zeta), h(z_coeffs, zeta * w % R)
    a, b = zv, zr
    for j in range(t):
        a = a * ((f[j] + beta * c.ks[j] % R * zeta + gamma) % R) % R
        b = b * ((f[j] + beta * h(key[t + 2 + j], zeta) + gamma) % R) % R
    l0 = h([pow(c.n, R - 2, R)] * c.n, zeta)
    num = (gate + alpha * (a - b) + alpha * alpha % R * (zv - 1) % R * l0) % R
    return h(T, zeta) * (pow(zeta, c.n, R) - 1) % R == num
