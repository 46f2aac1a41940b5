"""Independent reference for the last round of a circuit's proof (kzg_circuit_open, kzg_circuit_linearise, kzg_circuit_verify;
DESIGN.md section 4.23), in Python integers mod r, on top of circuit_oracle, ntt_oracle and open_sets_oracle.

With the evaluations abar_j = f_j(zeta), sbar_j = sigma_j(zeta) (j < t - 1), zw = z(zeta w), and
A = prod_(j<t) (abar_j + beta k_j zeta + gamma), B = zw prod_(j<t-1) (abar_j + beta sbar_j + gamma), Z = zeta^n - 1, l = L_0(zeta):

    r(X) = sum_j abar_j q_j(X) + abar_0 abar_1 q_M(X) + q_C(X) + (alpha A + alpha^2 l) z(X) - alpha beta B sigma_(t-1)(X)
           - Z sum_(c<e-1) zeta^(c n) T_c(X) + [ PI(zeta) - alpha B (abar_(t-1) + gamma) - alpha^2 l ]

  * coefficients    the coefficient vectors of the key, the wires, z and PI (ntt_oracle.intt)
  * evaluations     (abar, sbar, zw) by Horner
  * l0_at           L_0(zeta) by the POLYNOMIAL rule, (1 / n)(1 + zeta + .. + zeta^(n-1)): no division, so zeta in H needs no case
  * terms           r as a list of (scalar, name) with the constant; linearisation: r's n coefficients from it
  * stack           the 2 t + 1 polynomials [ r | f | sigma_0 .. sigma_(t-2) | z ] with set_of, the sets {zeta}, {zeta w}, the values
  * r_scalar        the scalar of [r] from the commitments' scalars: the verifier's combination
"""
import ntt_oracle as NO
import perm_quotient_oracle as PQ

R = PQ.R


def coefficients(c, z):
    """(key: the 2 t + 2 columns in the key's order, wires, z, PI or None) as coefficient vectors"""
    return ([NO.intt(col) for col in c.key_columns()], [NO.intt(col) for col in c.wires], NO.intt(z),
            None if c.pi is None else NO.intt(c.pi))


def chunks(T, n, log_ext):
    """T's e - 1 chunks of n coefficients, padded with zeros"""
    e = 1 << log_ext
    assert len(T) <= (e - 1) * n
    full = list(T) + [0] * ((e - 1) * n - len(T))
    return [full[k * n:(k + 1) * n] for k in range(e - 1)]


def l0_at(n, zeta):
    return PQ.horner([pow(n, R - 2, R)] * n, zeta)


def evaluations(c, coefs, zeta):
    key, wires, zc, _ = coefs
    t = c.t
    w = NO.domain_root(NO.log2_exact(c.n))
    return ([PQ.horner(f, zeta) for f in wires], [PQ.horner(key[t + 2 + j], zeta) for j in range(t - 1)], PQ.horner(zc, zeta * w % R))


def terms(c, coefs, log_ext, alpha, beta, gamma, zeta, evals=None, pi_zeta=None):
    """([(scalar, name)], constant): names ("key", j), ("z",), ("T", c); evals, pi_zeta: the verifier's inputs instead of the truth"""
    n, t, e = c.n, c.t, 1 << log_ext
    abar, sbar, zw = evaluations(c, coefs, zeta) if evals is None else evals
    if pi_zeta is None:
        pi_zeta = 0 if coefs[3] is None else PQ.horner(coefs[3], zeta)
    A, B = 1, zw
    for j in range(t):
        A = A * ((abar[j] + beta * c.ks[j] % R * zeta + gamma) % R) % R
    for j in range(t - 1):
        B = B * ((abar[j] + beta * sbar[j] + gamma) % R) % R
    Z, l = (pow(zeta, n, R) - 1) % R, l0_at(n, zeta)
    out = [(abar[j], ("key", j)) for j in range(t)]
    out += [(abar[0] * abar[1] % R, ("key", t)), (1, ("key", t + 1))]
    out += [((alpha * A + alpha * alpha % R * l) % R, ("z",))]
    out += [((-alpha * beta % R * B) % R, ("key", 2 * t + 1))]
    out += [((-Z * pow(zeta, k * n, R)) % R, ("T", k)) for k in range(e - 1)]
    return out, (pi_zeta - alpha * B % R * (abar[t - 1] + gamma) - alpha * alpha % R * l) % R


def linearisation(c, coefs, T, log_ext, alpha, beta, gamma, zeta):
    """r's n coefficients"""
    key, _, zc, _ = coefs
    tc = chunks(T, c.n, log_ext)
    cols = {("z",): zc}
    cols.update({("key", j): key[j] for j in range(2 * c.t + 2)})
    cols.update({("T", k): tc[k] for k in range(len(tc))})
    sc, const = terms(c, coefs, log_ext, alpha, beta, gamma, zeta)
    r = [sum(s * cols[name][i] for s, name in sc) % R for i in range(c.n)]
    r[0] = (r[0] + const) % R
    return r


def stack(c, coefs, r, zeta):
    """(polys, set_of, sets, ys) of the opening: [ r | f_0 .. f_(t-1) | sigma_0 .. sigma_(t-2) | z ] on {zeta}, {zeta w}"""
    key, wires, zc, _ = coefs
    t = c.t
    abar, sbar, zw = evaluations(c, coefs, zeta)
    w = NO.domain_root(NO.log2_exact(c.n))
    polys = [list(r)] + wires + [key[t + 2 + j] for j in range(t - 1)] + [zc]
    return polys, [0] * (2 * t) + [1], [[zeta % R], [zeta * w % R]], [[0]] + [[a] for a in abar] + [[s] for s in sbar] + [[zw]]


def public_input_at(n, public, zeta):
    """PI(zeta) = sum_i PI_i L_i(zeta) for the values at rows 0 .. len(public) - 1, the later rows zero; every L_i by the polynomial
    rule L_i(X) = L_0(X / w^i)"""
    w = NO.domain_root(NO.log2_exact(n))
    return sum(p * l0_at(n, zeta * pow(w, -i, R) % R) for i, p in enumerate(public)) % R


def r_scalar(c, coefs, log_ext, alpha, beta, gamma, zeta, evals, public, key_scalars, z_scalar, t_scalars):
    """the scalar of [r] = sum scalar [commitment] + const G from the scalars of the key's, z's and the chunks' commitments"""
    at = {("z",): z_scalar}
    at.update({("key", j): key_scalars[j] for j in range(2 * c.t + 2)})
    at.update({("T", k): t_scalars[k] for k in range(len(t_scalars))})
    sc, const = terms(c, coefs, log_ext, alpha, beta, gamma, zeta, evals, public_input_at(c.n, public, zeta))
    return (sum(s * at[name] for s, name in sc) + const) % R
