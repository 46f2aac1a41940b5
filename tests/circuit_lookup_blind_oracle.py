"""Independent reference for zero-knowledge lookup proofs (kzg_circuit_lookup_quotient_blinded, kzg_circuit_lookup_prove_blinded;
DESIGN.md section 4.30), in Python integers mod r, on top of circuit_lookup_oracle, blind_oracle and circuit_lookup_cases.build.

With Z_H = X^n - 1, e = 2^log_ext, blind_oracle's blinders b_j (two per wire), c (three), d_0 .. d_(e-3) and two new groups p (three)
and u (two):

    f~_j, z~, T~_c as blind_oracle;     phi~ = phi + (p_0 + p_1 X + p_2 X^2) Z_H;     m~ = m + (u_0 + u_1 X) Z_H
    F~ = beta + q_K sum_(j<c) theta^j f~_j,  Tt = beta + sum_j theta^j tab_j
    G'~ = alpha^3 [ (phi~(w X) - phi~) F~ Tt - Tt + m~ F~ ] + alpha^4 L_0 phi~
    T~ = (Num(f~, z~) + G'~) / Z_H, with D = max(t n + t + 3, 3 n + 2) coefficients, returned as L_T = (e - 1) n + t + 3

  * Blinders            the five groups, flat() in the order of the library's array: b, c, d, p, u; zero(), random()
  * shape_ok, keep      the shape rule and D
  * full_degree_variant, case   circuit_lookup_cases' case of a shape with the table's rows in an order of full degree, so that T~ has
                        exactly D coefficients and not fewer (the table of the shared (4, 2, 1, 2) case has degree n - 2)
  * coefficients        a Coefs: blind_oracle.coefficients' tuple, m~, phi~, the table's and q_K's coefficient vectors
  * gprime_coeffs       G'~ as coefficients: products of values over a SUBGROUP of at least 4 n + 2 points, one inverse transform
  * quotient            T~ by exact division (asserts a zero remainder and the length D), padded to L_T
  * lookup_evaluations  (tbar, qbar, phi~(zeta w)) by Horner; evaluations: blind_oracle's (abar, sbar, z~(zeta w))
  * linearisation       r~_L's n + t + 3 coefficients from given chunks
  * stack               the 2 t + c + 3 polynomials of the opening, each padded to n + t + 3
  * prove               the proof bytes under a known secret, mirroring circuit_lookup_oracle.prove
"""
import random

import blind_oracle as BO
import circuit_lookup_oracle as CL
import circuit_oracle as CO
import linearise_oracle as LN
import lookup_oracle as LO
import ntt_oracle as NO
import open_sets_oracle as SO
import perm_quotient_oracle as PQ
import transcript_oracle as TR
import trapdoor_oracle as TO

R = PQ.R


class Blinders(BO.Blinders):
    def __init__(self, b, c, d, p, u):
        BO.Blinders.__init__(self, b, c, d)
        self.p, self.u = list(p), list(u)
        assert len(self.p) == 3 and len(self.u) == 2

    def flat(self):
        return BO.Blinders.flat(self) + self.p + self.u

    def generic(self):
        """every leading blinder is non-zero: the blinded polynomials have their full degrees"""
        return all(pair[1] for pair in self.b) and self.c[2] != 0 and self.p[2] != 0 and self.u[1] != 0

    def copy(self):
        return Blinders(self.b, self.c, self.d, self.p, self.u)

    @staticmethod
    def zero(t, log_ext):
        base = BO.Blinders.zero(t, log_ext)
        return Blinders(base.b, base.c, base.d, [0, 0, 0], [0, 0])

    @staticmethod
    def random(t, log_ext, seed):
        base = BO.Blinders.random(t, log_ext, seed)
        rnd = random.Random(77000 + seed)
        return Blinders(base.b, base.c, base.d, [1 + rnd.randrange(R - 1) for _ in range(3)], [1 + rnd.randrange(R - 1) for _ in range(2)])


def keep(n, t):
    """D: the coefficients of T~"""
    return max(t * n + t + 3, 3 * n + 2)


def shape_ok(n, t, c, log_ext):
    e = 1 << log_ext
    return (1 <= c <= t and e >= max(t + 1, 4) and 3 * t + e + c + 5 <= 32 and keep(n, t) < e * n and
            keep(n, t) <= BO.quotient_len(n, t, log_ext))


def full_degree_variant(lc):
    """lc, or lc with the table's rows in another order (the lookup holds for any order) such that the first table column's
    interpolant has degree n - 1: a table like [0, a, 0, a] at n = 4 interpolates to degree n - 2, and T~ then stays below D"""
    n = lc.n
    rows = list(zip(*lc.table))
    orders = [rows, sorted(rows), sorted(rows, reverse=True)] + [rows[k:] + rows[:k] for k in range(1, n)]
    for order in orders:
        table = [[row[j] for row in order] for j in range(lc.c)]
        if NO.intt(list(table[0]))[n - 1] != 0:
            return lc if order is rows else CL.LookupCircuit(lc.circuit, table, lc.q_lookup)
    raise AssertionError("no order of the table's rows has full degree")


class Case:
    """circuit_lookup_cases' case of a shape with a table of full degree: lc, the columns m and phi over H and the accumulator z
    under circuit_lookup_cases' challenges; plain: the unchanged case"""

    def __init__(self, n, t, c, log_ext, with_pi=True):
        import circuit_lookup_cases as CC
        self.plain = CC.case(n, t, c, log_ext, with_pi)
        self.n, self.t, self.c, self.log_ext = n, t, c, log_ext
        self.lc, self.z = full_degree_variant(self.plain.lc), self.plain.z
        self.m, self.phi = self.plain.m, self.plain.phi
        if self.lc is not self.plain.lc:
            _, _, self.m, self.phi, last, missing = CL.columns(self.lc, CC.THETA, CC.BETA)
            assert missing is None and last == 0
        self.challenges = (CC.THETA, CC.BETA, CC.GAMMA, CC.ALPHA)


def case(n, t, c, log_ext, with_pi=True):
    import circuit_lookup_cases as CC
    return CC.memo(("blinded lookup case", n, t, c, log_ext, with_pi), lambda: Case(n, t, c, log_ext, with_pi))


class Coefs:
    """base: blind_oracle.coefficients' (key, f~, z~, PI); m, phi: m~ and phi~; table, qk: the key's lookup columns"""

    def __init__(self, base, m, phi, table, qk):
        self.base, self.m, self.phi, self.table, self.qk = base, m, phi, table, qk


def coefficients(lc, z, m, phi, bl):
    n = lc.n
    return Coefs(BO.coefficients(lc.circuit, z, bl), BO.blind(NO.intt(list(m)), bl.u, n), BO.blind(NO.intt(list(phi)), bl.p, n),
                 [NO.intt(list(col)) for col in lc.table], NO.intt(list(lc.q_lookup)))


def gprime_coeffs(lc, cf, theta, beta, alpha):
    """G'~ as coefficients, trailing zeros trimmed.  Degrees: phi~ n + 2, F~ 2 n, Tt n - 1, so Lk1 4 n + 1, m~ F~ 3 n + 1, Lk2 2 n + 1"""
    n = lc.n
    assert len(cf.phi) == n + 3 and len(cf.m) == n + 2 and all(len(f) == n + 2 for f in cf.base[1])
    M = 4
    while M < 4 * n + 2:
        M *= 2
    on = lambda coef: NO.ntt(list(coef) + [0] * (M - len(coef)))
    fv = [on(f) for f in cf.base[1][:lc.c]]
    tv = [on(col) for col in cf.table]
    qk, mv = on(cf.qk), on(cf.m)
    pv = on(cf.phi)
    pr = pv[M // n:] + pv[:M // n]  # phi~(w X) at the subgroup's point i is phi~ at its point i + M / n
    l0 = on([pow(n, R - 2, R)] * n)
    a3 = pow(alpha, 3, R)
    a4 = a3 * alpha % R
    vals = []
    for i in range(M):
        F = (beta + qk[i] * CL._folded(fv, theta, i)) % R
        Tt = (beta + CL._folded(tv, theta, i)) % R
        lk1 = ((pr[i] - pv[i]) * F % R * Tt - Tt + mv[i] * F) % R
        vals.append((a3 * lk1 + a4 * l0[i] % R * pv[i]) % R)
    out = PQ._trim(NO.intt(vals))
    assert len(out) <= 4 * n + 2
    return out


def numerator(lc, cf, theta, beta, gamma, alpha):
    """Num_L = Num(f~, z~) + G'~ as coefficients"""
    a, b = BO.numerator(lc.circuit, cf.base, alpha, beta, gamma), gprime_coeffs(lc, cf, theta, beta, alpha)
    L = max(len(a), len(b))
    return PQ._trim([(x + y) % R for x, y in zip(a + [0] * (L - len(a)), b + [0] * (L - len(b)))])


def quotient(lc, cf, log_ext, theta, beta, gamma, alpha, exact=True, full_degree=False):
    """T~ padded to L_T coefficients; exact: assert a zero remainder (else return (T~ unpadded, remainder)); full_degree: assert that
    T~ has exactly D coefficients (generic blinders at n > 2: at n <= 2, w^(n + 2) = 1 and the leading terms cancel)"""
    n, t = lc.n, lc.t
    T, rem = PQ.divide_vanishing(numerator(lc, cf, theta, beta, gamma, alpha), n)
    if not exact:
        return T, rem
    assert rem == [], "Num_L(f~, z~, phi~, m~) is not divisible by X^n - 1"
    T = PQ._trim(T)
    D, LT = keep(n, t), BO.quotient_len(n, t, log_ext)
    assert len(T) <= D <= LT and D < (n << log_ext)
    if full_degree:
        assert len(T) == D, (len(T), D)
    return T + [0] * (LT - len(T))


def chunks(T, n, t, log_ext, bl):
    return BO.chunks(T, n, t, log_ext, bl)


def evaluations(lc, cf, zeta):
    return BO.evaluations(lc.circuit, cf.base, zeta)


def lookup_evaluations(lc, cf, zeta):
    """(tbar_0 .. tbar_(c-1), qbar, phi~(zeta w)) by Horner"""
    w = NO.domain_root(NO.log2_exact(lc.n))
    return [PQ.horner(col, zeta) for col in cf.table], PQ.horner(cf.qk, zeta), PQ.horner(cf.phi, zeta * w % R)


def linearisation(lc, cf, tc, log_ext, theta, beta, gamma, alpha, zeta):
    """r~_L's n + t + 3 coefficients: r_L's formula with z~, phi~, m~, the chunks tc and the blinded evaluations"""
    c = lc.circuit
    key, _, zc, _ = cf.base
    n, t = c.n, c.t
    L = n + t + 3
    cols = {("z",): zc}
    cols.update({("key", j): key[j] for j in range(2 * t + 2)})
    cols.update({("T", k): tc[k] for k in range(len(tc))})
    sc, const = LN.terms(c, cf.base, log_ext, alpha, beta, gamma, zeta)
    abar, _, _ = evaluations(lc, cf, zeta)
    tbar, qbar, phiw = lookup_evaluations(lc, cf, zeta)
    on_phi, on_m, more = CL.lookup_terms(lc, theta, beta, alpha, zeta, abar, tbar, qbar, phiw)
    r = [0] * L
    for s, col in [(s, cols[name]) for s, name in sc] + [(on_phi, cf.phi), (on_m, cf.m)]:
        assert len(col) <= L
        for i, v in enumerate(col):
            r[i] = (r[i] + s * v) % R
    r[0] = (r[0] + const + more) % R
    return r


def stack(lc, cf, r_l, zeta):
    """(polys, set_of, sets, ys): [ r~_L | f~ | sigma_0 .. sigma_(t-2) | z~ | tab_0 .. tab_(c-1) | q_K | phi~ ], each padded to n + t + 3"""
    L = lc.n + lc.t + 3
    polys, set_of, sets, ys = BO.stack(lc.circuit, cf.base, r_l, zeta)
    tbar, qbar, phiw = lookup_evaluations(lc, cf, zeta)
    polys = polys + [list(p) + [0] * (L - len(p)) for p in cf.table + [cf.qk, cf.phi]]
    return polys, set_of + [0] * (lc.c + 1) + [1], sets, ys + [[v] for v in tbar] + [[qbar], [phiw]]


def prove(oracle, lc, log_ext, bl, secret, n_public=None, chunk_bl=None):
    """The blinded proof of a lookup circuit under a known secret, in circuit_lookup_oracle.prove's format and transcript.
    chunk_bl: other blinders for the COMMITTED chunks than those r~_L is formed with (a proof the verifier must reject).
    Returns a dict: proof (bytes), key48, public, the challenges and every intermediate"""
    c = lc.circuit
    n, t = c.n, c.t
    assert shape_ok(n, t, lc.c, log_ext)
    g = lambda s: TO.g1_scalar(oracle, s)
    com = lambda coef: g(PQ.horner(coef, secret))
    public = TR.public_of(c, n_public)
    key_s = CL.key_scalars(lc, secret)
    key48 = [g(s) for s in key_s]
    h = CL.statement_hash(n, t, log_ext, lc.c, c.ks, key48, public)
    wires = [BO.blind(NO.intt(col), b, n) for col, b in zip(c.wires, bl.b)]
    out = b"".join(com(w) for w in wires)
    h = TR.absorb(h, out)
    theta = TR.challenge(h)
    f, T_ = CL.fold(lc, theta)
    m, _, missing = LO.multiplicities(T_, [f])
    assert missing is None, "a tuple is in no table row"
    out += com(BO.blind(NO.intt(list(m)), bl.u, n))
    h = TR.absorb(h, out[-48:])
    beta, gamma = TR.challenge(h, 0), TR.challenge(h, 1)
    a, b = LO.lookup_columns([f], T_, m, beta)
    phi, last = LO.direct(a, b)
    assert last == 0, "the lookup does not hold"
    z, zlast = CO.z_of(c, beta, gamma)
    assert zlast == 1, "the copy constraints do not hold"
    cf = coefficients(lc, z, m, phi, bl)
    assert cf.base[1] == wires
    out += com(cf.base[2]) + com(cf.phi)
    h = TR.absorb(h, out[-96:])
    alpha = TR.challenge(h)
    T = quotient(lc, cf, log_ext, theta, beta, gamma, alpha)
    tc = chunks(T, n, t, log_ext, bl)
    t48 = b"".join(com(ch) for ch in (tc if chunk_bl is None else chunks(T, n, t, log_ext, chunk_bl)))
    out += t48
    h = TR.absorb(h, t48)
    zeta = TR.challenge(h)
    r_l = linearisation(lc, cf, tc, log_ext, theta, beta, gamma, alpha, zeta)
    assert len(r_l) == n + t + 3 and PQ.horner(r_l, zeta) == 0
    polys, set_of, sets, ys = stack(lc, cf, r_l, zeta)
    evals = [y[0] for y in ys[1:]]
    ev = b"".join(TR.fr_bytes(x) for x in evals)
    out += ev
    h = TR.absorb(h, ev)
    v = TR.challenge(h)
    w = SO.proof_scalar(polys, set_of, sets, v, secret)
    out += g(w)
    assert len(out) == CL.proof_size(t, log_ext, lc.c)
    assert CL.challenges(n, t, log_ext, lc.c, c.ks, key48, public, out) == (theta, beta, gamma, alpha, zeta, v)
    return dict(proof=out, lc=lc, log_ext=log_ext, bl=bl, key48=key48, key_s=key_s, public=public, theta=theta, beta=beta, gamma=gamma,
                alpha=alpha, zeta=zeta, v=v, z=z, m=m, phi=phi, cf=cf, T=T, chunks=tc, r_l=r_l, evals=evals, w=w)
