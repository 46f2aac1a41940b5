"""Independent reference for zero-knowledge circuit proofs (kzg_blind_evaluations .. kzg_circuit_open_blinded; DESIGN.md section
4.24), in Python integers mod r, on top of circuit_oracle, linearise_oracle, perm_quotient_oracle and ntt_oracle.

With Z_H = X^n - 1, e = 2^log_ext and the blinders b_j (two per wire), c (three), d_0 .. d_(e-3):

    f~_j = f_j + (b_j0 + b_j1 X) Z_H,     z~ = z + (c_0 + c_1 X + c_2 X^2) Z_H,     T~ = Num(f~, z~) / Z_H   (degree t n + t + 2)
    T~_c = T_c + d_c X^n - d_(c-1)  (d_(-1) = d_(e-2) = 0),  T_c = coefficients [c n, (c + 1) n) of T~, the last one up to L_T

  * Blinders            the three groups, flat() in the order of the library's array; zero(), random()
  * blind               f + b Z_H as n + len(b) coefficients
  * coefficients        linearise_oracle.coefficients with the wires and z blinded
  * numerator           Num(f~, z~) as coefficients: products of values over a SUBGROUP large enough for its degree, one inverse
                        transform -- no coset, no division
  * quotient            T~ by exact division (asserts a zero remainder and the degree), padded to L_T
  * chunks              the e - 1 blinded chunks (all but the last of n + 1 coefficients, the last of n + t + 3)
  * evaluations         (abar, sbar, zw) of the blinded polynomials by Horner
  * linearisation       r~'s n + t + 3 coefficients, from linearise_oracle.terms with the blinded evaluations
  * stack               [ r~ | f~ | sigma_0 .. sigma_(t-2) | z~ ], each padded to n + t + 3, with set_of, the sets and the values
  * proof_case          everything the verifier is handed, as scalars under a known secret (trapdoor_oracle's world)
"""
import random

import circuit_oracle as CO
import linearise_oracle as LO
import ntt_oracle as NO
import open_sets_oracle as SO
import perm_quotient_oracle as PQ

R = PQ.R


class Blinders:
    def __init__(self, b, c, d):
        self.b, self.c, self.d = [list(x) for x in b], list(c), list(d)

    def flat(self):
        return [v for pair in self.b for v in pair] + self.c + self.d

    @staticmethod
    def zero(t, log_ext):
        return Blinders([[0, 0]] * t, [0, 0, 0], [0] * ((1 << log_ext) - 2))

    @staticmethod
    def random(t, log_ext, seed):
        rnd = random.Random(9000 + seed)
        return Blinders([[rnd.randrange(R), rnd.randrange(R)] for _ in range(t)], [rnd.randrange(R) for _ in range(3)],
                        [rnd.randrange(R) for _ in range((1 << log_ext) - 2)])


def shape_ok(n, t, log_ext):
    return (n << log_ext) >= t * n + t + 4 and t + 1 <= (1 << log_ext)


def quotient_len(n, t, log_ext):
    return ((1 << log_ext) - 1) * n + t + 3


def blind(coeffs, b, n):
    """f + b(X) (X^n - 1): n + len(b) coefficients (at n < len(b) the two ranges overlap)"""
    assert len(coeffs) == n
    out = list(coeffs) + [0] * len(b)
    for i, v in enumerate(b):
        out[i] = (out[i] - v) % R
        out[n + i] = (out[n + i] + v) % R
    return out


def coefficients(c, z, bl):
    """(key, f~, z~, PI or None) as coefficient vectors"""
    key, wires, zc, pi = LO.coefficients(c, z)
    return key, [blind(f, b, c.n) for f, b in zip(wires, bl.b)], blind(zc, bl.c, c.n), pi


def numerator(c, coefs, alpha, beta, gamma):
    """Num(f~, z~) as coefficients, trailing zeros trimmed"""
    key, wires, zc, pi = coefs
    n, t = c.n, c.t
    w = NO.domain_root(NO.log2_exact(n))
    M = 4  # above deg Num: the permutation's (t + 1) n + t + 2, the gate's 3 n + 1
    while M < max((t + 1) * n + t + 3, 3 * n + 2):
        M *= 2
    wM = NO.domain_root(NO.log2_exact(M))
    on = lambda cf: NO.ntt(list(cf) + [0] * (M - len(cf)))
    f = [on(x) for x in wires]
    q = [on(x) for x in key]
    zv = on(zc)
    zr = on([v * pow(w, i, R) % R for i, v in enumerate(zc)])  # z~(w X)
    l0 = on([pow(n, R - 2, R)] * n)
    pv = on(pi) if pi is not None else [0] * M
    vals, x = [], 1
    for i in range(M):
        gate = q[t][i] * f[0][i] % R * f[1][i] + q[t + 1][i] + pv[i]
        a, b = zv[i], zr[i]
        for j in range(t):
            gate += q[j][i] * f[j][i]
            a = a * ((f[j][i] + beta * c.ks[j] % R * x + gamma) % R) % R
            b = b * ((f[j][i] + beta * q[t + 2 + j][i] + gamma) % R) % R
        vals.append((gate + alpha * (a - b) + alpha * alpha % R * (zv[i] - 1) % R * l0[i]) % R)
        x = x * wM % R
    return PQ._trim(NO.intt(vals))


def quotient(c, coefs, log_ext, alpha, beta, gamma, exact=True):
    """T~ padded to L_T coefficients; exact: assert a zero remainder (else return (T~ unpadded, remainder))"""
    T, rem = PQ.divide_vanishing(numerator(c, coefs, alpha, beta, gamma), c.n)
    if not exact:
        return T, rem
    assert rem == [], "Num(f~, z~) is not divisible by X^n - 1"
    T = PQ._trim(T)
    assert len(T) <= c.t * c.n + c.t + 3
    LT = quotient_len(c.n, c.t, log_ext)
    return T + [0] * (LT - len(T))


def plain_chunks(T, n, t, log_ext):
    """T_c: coefficients [c n, (c + 1) n), the last chunk everything from (e - 2) n to L_T"""
    e = 1 << log_ext
    assert len(T) == quotient_len(n, t, log_ext)
    return [T[k * n:(k + 1) * n] for k in range(e - 2)] + [T[(e - 2) * n:]]


def chunks(T, n, t, log_ext, bl):
    """T~_c = T_c + d_c X^n - d_(c-1)"""
    e = 1 << log_ext
    out = [list(ch) for ch in plain_chunks(T, n, t, log_ext)]
    for k in range(e - 1):
        if k >= 1:
            out[k][0] = (out[k][0] - bl.d[k - 1]) % R
        if k < e - 2:
            out[k] = out[k] + [bl.d[k]]
    return out


def evaluations(c, coefs, zeta):
    return LO.evaluations(c, coefs, zeta)


def linearisation(c, coefs, T, log_ext, bl, alpha, beta, gamma, zeta, evals=None):
    """r~'s n + t + 3 coefficients: r's formula with z~, the T~_c and the blinded evaluations"""
    key, _, zc, _ = coefs
    n, t = c.n, c.t
    L = n + t + 3
    tc = chunks(T, n, t, log_ext, bl)
    cols = {("z",): zc}
    cols.update({("key", j): key[j] for j in range(2 * t + 2)})
    cols.update({("T", k): tc[k] for k in range(len(tc))})
    sc, const = LO.terms(c, coefs, log_ext, alpha, beta, gamma, zeta, evals=evals)
    r = [0] * L
    for s, name in sc:
        for i, v in enumerate(cols[name]):
            r[i] = (r[i] + s * v) % R
    r[0] = (r[0] + const) % R
    return r


def stack(c, coefs, r, zeta):
    """(polys, set_of, sets, ys): every polynomial zero-padded to n + t + 3 coefficients"""
    polys, set_of, sets, ys = LO.stack(c, coefs, r, zeta)
    L = c.n + c.t + 3
    return [list(p) + [0] * (L - len(p)) for p in polys], set_of, sets, ys


def proof_case(c, z, log_ext, bl, alpha, beta, gamma, zeta, v, secret):
    """the prover's outputs and the scalars of every commitment under the secret"""
    coefs = coefficients(c, z, bl)
    key, wires, zc, _ = coefs
    T = quotient(c, coefs, log_ext, alpha, beta, gamma)
    tc = chunks(T, c.n, c.t, log_ext, bl)
    r = linearisation(c, coefs, T, log_ext, bl, alpha, beta, gamma, zeta)
    polys, set_of, sets, ys = stack(c, coefs, r, zeta)
    return dict(c=c, coefs=coefs, T=T, chunks=tc, r=r, polys=polys, set_of=set_of, sets=sets, ys=ys, log_ext=log_ext, zeta=zeta, v=v,
                evals=evaluations(c, coefs, zeta), key_s=[PQ.horner(col, secret) for col in key],
                wire_s=[PQ.horner(col, secret) for col in wires], z_s=PQ.horner(zc, secret),
                t_s=[PQ.horner(ch, secret) for ch in tc], w=SO.proof_scalar(polys, set_of, sets, v, secret))
