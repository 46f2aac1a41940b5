"""Independent references for the lookup argument of a circuit whose key holds a table (kzg_circuit_create_lookup,
kzg_circuit_lookup_columns, kzg_circuit_lookup_quotient), in Python integers mod r, on top of
circuit_oracle, lookup_oracle, perm_quotient_oracle and ntt_oracle.

A lookup circuit is a circuit_oracle.Circuit with c <= t table columns tab_j and a selector q_K (n values each).  With theta, beta:

    f_i = q_K[i] sum_j theta^j f_j[i]        T_i = sum_j theta^j tab_j[i]
    m   = lookup_oracle.multiplicities of the column f in the column T (the count at the LEAST row)
    phi = lookup_oracle.direct of the lookup form: phi_(i+1) = phi_i + 1 / (beta + f_i) - m_i / (beta + T_i)
    F = beta + q_K sum_j theta^j f_j,  Tt = beta + sum_j theta^j tab_j    (polynomials)
    G' = alpha^3 [ (phi(w X) - phi(X)) F Tt - Tt + m F ] + alpha^4 L_0 phi

  * fold            (f, T) over H
  * columns         (f, T, m, phi, phi_n, missing): missing is the least row whose folded tuple is in no table row, or None
  * gprime_coeffs   G' as coefficients: products of values over a SUBGROUP of at least 4 n points, one inverse transform -- no
                    coset, no division
  * quotient        circuit_oracle.quotient(extra = G'), asserting a zero remainder; remainder: the same division's remainder
  * check_at        T(zeta) (zeta^n - 1) == Num(zeta) + G'(zeta), G' from its DEFINITION at zeta by Horner (not from gprime_coeffs)
  * linearisation   r_L's n coefficients; stack: the 2 t + c + 3 polynomials of the opening with their sets and values
  * statement_hash, challenges, layout, split   the transcript ("kzg_mi355x/plonk-lookup/v1") and the proof's seven fields
  * prove           the proof bytes under a known secret (trapdoor_oracle's world), mirroring transcript_oracle.prove
"""
import hashlib

import circuit_oracle as CO
import linearise_oracle as LN
import lookup_oracle as LO
import ntt_oracle as NO
import open_sets_oracle as SO
import perm_quotient_oracle as PQ
import transcript_oracle as TR
import trapdoor_oracle as TO

R = PQ.R


class LookupCircuit:
    """circuit: a circuit_oracle.Circuit; table: c columns of n integers; q_lookup: n integers"""

    def __init__(self, circuit, table, q_lookup):
        self.circuit, self.table, self.q_lookup = circuit, table, q_lookup
        self.n, self.t, self.c = circuit.n, circuit.t, len(table)
        assert 1 <= self.c <= self.t

    def key_columns(self):
        """the 2 t + c + 3 resident columns in the order of the key: circuit_oracle's, then tab[0..c), q_K"""
        return self.circuit.key_columns() + list(self.table) + [self.q_lookup]


def _folded(cols, theta, i):
    acc, p = 0, 1
    for col in cols:
        acc = (acc + p * col[i]) % R
        p = p * theta % R
    return acc


def fold(lc, theta, wires=None, table=None):
    f = lc.circuit.wires if wires is None else wires
    tab = lc.table if table is None else table
    return ([lc.q_lookup[i] * _folded(f[:lc.c], theta, i) % R for i in range(lc.n)], [_folded(tab, theta, i) for i in range(lc.n)])


def columns(lc, theta, beta, wires=None, table=None):
    f, T = fold(lc, theta, wires, table)
    m, _, missing = LO.multiplicities(T, [f])
    if missing is not None:
        return f, T, m, None, None, missing
    a, b = LO.lookup_columns([f], T, m, beta)
    phi, last = LO.direct(a, b)
    return f, T, m, phi, last, None


def gprime_coeffs(lc, theta, beta, alpha, m, phi, wires=None, table=None):
    """G' as coefficients (trailing zeros trimmed); m, phi: n values over H each"""
    f = lc.circuit.wires if wires is None else wires
    tab = lc.table if table is None else table
    n = lc.n
    M = 4
    while M < 4 * n:
        M *= 2
    w = NO.domain_root(NO.log2_exact(n))
    on_c = lambda coef: NO.ntt(list(coef) + [0] * (M - len(coef)))
    on = lambda vals: on_c(NO.intt(list(vals)))
    fv = [on(col) for col in f[:lc.c]]
    tv = [on(col) for col in tab]
    qk, mv = on(lc.q_lookup), on(m)
    pc = NO.intt(list(phi))
    pv, pr = on_c(pc), on_c([c * pow(w, i, R) % R for i, c in enumerate(pc)])  # phi(X), phi(w X)
    l0 = on_c([pow(n, R - 2, R)] * n)
    a3 = pow(alpha, 3, R)
    a4 = a3 * alpha % R
    vals = []
    for i in range(M):
        F = (beta + qk[i] * _folded(fv, theta, i)) % R
        Tt = (beta + _folded(tv, theta, i)) % R
        lk1 = ((pr[i] - pv[i]) * F % R * Tt - Tt + mv[i] * F) % R
        vals.append((a3 * lk1 + a4 * l0[i] % R * pv[i]) % R)
    return PQ._trim(NO.intt(vals))


def quotient(lc, z, theta, beta, gamma, alpha, m, phi, wires=None, table=None):
    """T of the lookup circuit, asserting a zero remainder"""
    return CO.quotient(lc.circuit, z, alpha, beta, gamma, wires, extra=gprime_coeffs(lc, theta, beta, alpha, m, phi, wires, table))


def remainder(lc, z, theta, beta, gamma, alpha, m, phi, wires=None, table=None):
    return CO.remainder(lc.circuit, z, alpha, beta, gamma, wires, extra=gprime_coeffs(lc, theta, beta, alpha, m, phi, wires, table))


def gprime_at(lc, zeta, theta, beta, alpha, m, phi, wires=None):
    """G'(zeta) from the definition, every polynomial by Horner from its interpolant"""
    f = lc.circuit.wires if wires is None else wires
    h = lambda vals, x=zeta: PQ.horner(NO.intt(list(vals)), x)
    w = NO.domain_root(NO.log2_exact(lc.n))
    fz = [h(col) for col in f[:lc.c]]
    tz = [h(col) for col in lc.table]
    F = (beta + h(lc.q_lookup) * sum(pow(theta, j, R) * v for j, v in enumerate(fz))) % R
    Tt = (beta + sum(pow(theta, j, R) * v for j, v in enumerate(tz))) % R
    pz, pw = h(phi), h(phi, zeta * w % R)
    l0 = PQ.horner([pow(lc.n, R - 2, R)] * lc.n, zeta)
    lk1 = ((pw - pz) * F % R * Tt - Tt + h(m) * F) % R
    return (pow(alpha, 3, R) * lk1 + pow(alpha, 4, R) * l0 % R * pz) % R


def check_at(zeta, T, lc, z, theta, beta, gamma, alpha, m, phi):
    """T(zeta) (zeta^n - 1) == Num_L(zeta), with G'(zeta) handed to circuit_oracle.check_at as a constant polynomial"""
    c = lc.circuit
    g = gprime_at(lc, zeta, theta, beta, alpha, m, phi)
    return CO.check_at(zeta, T, c, [NO.intt(col) for col in c.wires], NO.intt(list(z)), alpha, beta, gamma, extra=[g])


# ---- the last round and the proof bytes ------------------------------------------------------------------------------------------
# r_L(X) = r(X) + (alpha^4 l - alpha^3 F T) phi(X) + alpha^3 F m(X) + alpha^3 (phiw F T - T), with F = beta + qbar sum theta^j abar_j,
# T = beta + sum theta^j tbar_j, l = L_0(zeta) and r linearise_oracle's polynomial formed with the lookup circuit's quotient.
DST = b"kzg_mi355x/plonk-lookup/v1"
FIELDS = ("wires", "m", "z", "phi", "chunks", "evals", "w")


def lookup_evaluations(lc, phi, zeta):
    """(tbar_0 .. tbar_(c-1), qbar, phi(zeta w)) by Horner"""
    w = NO.domain_root(NO.log2_exact(lc.n))
    return ([PQ.horner(NO.intt(list(col)), zeta) for col in lc.table], PQ.horner(NO.intt(list(lc.q_lookup)), zeta),
            PQ.horner(NO.intt(list(phi)), zeta * w % R))


def lookup_terms(lc, theta, beta, alpha, zeta, abar, tbar, qbar, phiw):
    """(the scalar on phi(X), the scalar on m(X), the constant) that the lookup adds to r"""
    F = (beta + qbar * sum(pow(theta, j, R) * abar[j] for j in range(lc.c))) % R
    T = (beta + sum(pow(theta, j, R) * tbar[j] for j in range(lc.c))) % R
    a3, l = pow(alpha, 3, R), LN.l0_at(lc.n, zeta)
    return (a3 * alpha % R * l - a3 * F % R * T) % R, a3 * F % R, a3 * ((phiw * F % R * T - T) % R) % R


def linearisation(lc, z, T, log_ext, theta, beta, gamma, alpha, zeta, m, phi):
    """r_L's n coefficients"""
    c = lc.circuit
    coefs = LN.coefficients(c, z)
    r = LN.linearisation(c, coefs, T, log_ext, alpha, beta, gamma, zeta)
    abar, _, _ = LN.evaluations(c, coefs, zeta)
    tbar, qbar, phiw = lookup_evaluations(lc, phi, zeta)
    on_phi, on_m, const = lookup_terms(lc, theta, beta, alpha, zeta, abar, tbar, qbar, phiw)
    pc, mc = NO.intt(list(phi)), NO.intt(list(m))
    out = [(r[i] + on_phi * pc[i] + on_m * mc[i]) % R for i in range(lc.n)]
    out[0] = (out[0] + const) % R
    return out


def stack(lc, z, r_l, zeta, phi):
    """(polys, set_of, sets, ys): [ r_L | f | sigma_0 .. sigma_(t-2) | z | tab_0 .. tab_(c-1) | q_K | phi ], z and phi on {zeta w}"""
    c = lc.circuit
    coefs = LN.coefficients(c, z)
    polys, set_of, sets, ys = LN.stack(c, coefs, r_l, zeta)
    tbar, qbar, phiw = lookup_evaluations(lc, phi, zeta)
    polys = polys + [NO.intt(list(col)) for col in lc.table] + [NO.intt(list(lc.q_lookup)), NO.intt(list(phi))]
    return polys, set_of + [0] * (lc.c + 1) + [1], sets, ys + [[v] for v in tbar] + [[qbar], [phiw]]


def proof_size(t, log_ext, c):
    return 48 * (t + (1 << log_ext) + 3) + 32 * (2 * t + c + 2)


def layout(t, log_ext, c):
    """{field: (first byte, end)}"""
    e = 1 << log_ext
    sizes = (48 * t, 48, 48, 48, 48 * (e - 1), 32 * (2 * t + c + 2), 48)
    out, at = {}, 0
    for name, size in zip(FIELDS, sizes):
        out[name] = (at, at + size)
        at += size
    assert at == proof_size(t, log_ext, c)
    return out


def split(proof, t, log_ext, c):
    assert len(proof) == proof_size(t, log_ext, c)
    return {name: proof[a:b] for name, (a, b) in layout(t, log_ext, c).items()}


def statement_hash(n, t, log_ext, c, shifts, key48, public):
    assert len(shifts) == t and len(key48) == 2 * t + c + 3 and all(len(k) == 48 for k in key48)
    head = DST + b"".join(x.to_bytes(8, "big") for x in (n, t, log_ext, c, len(public)))
    return hashlib.sha256(head + b"".join(TR.fr_bytes(k) for k in shifts) + b"".join(key48) +
                          b"".join(TR.fr_bytes(p) for p in public)).digest()


def challenges(n, t, log_ext, c, shifts, key48, public, proof):
    """(theta, beta, gamma, alpha, zeta, v): the bytes are hashed as they are"""
    f = split(proof, t, log_ext, c)
    h = TR.absorb(statement_hash(n, t, log_ext, c, shifts, key48, public), f["wires"])
    theta = TR.challenge(h)
    h = TR.absorb(h, f["m"])
    beta, gamma = TR.challenge(h, 0), TR.challenge(h, 1)
    h = TR.absorb(h, f["z"] + f["phi"])
    alpha = TR.challenge(h)
    h = TR.absorb(h, f["chunks"])
    zeta = TR.challenge(h)
    h = TR.absorb(h, f["evals"])
    return theta, beta, gamma, alpha, zeta, TR.challenge(h)


def key_scalars(lc, secret):
    return [PQ.horner(NO.intt(list(col)), secret) for col in lc.key_columns()]


def prove(oracle, lc, log_ext, secret, n_public=None):
    """The proof of a lookup circuit under a known secret (every commitment is [P(s)]G), mirroring transcript_oracle.prove.  Returns
    a dict: proof (bytes), key48, public, the challenges and every intermediate"""
    c = lc.circuit
    n, t = c.n, c.t
    g = lambda s: TO.g1_scalar(oracle, s)
    com = lambda vals: g(PQ.horner(NO.intt(list(vals)), secret))
    public = TR.public_of(c, n_public)
    key_s = key_scalars(lc, secret)
    key48 = [g(s) for s in key_s]
    h = statement_hash(n, t, log_ext, lc.c, c.ks, key48, public)
    out = b"".join(com(col) for col in c.wires)
    h = TR.absorb(h, out)
    theta = TR.challenge(h)
    f, T_, m, _, _, missing = columns(lc, theta, 1)
    assert missing is None, "a tuple is in no table row"
    out += com(m)
    h = TR.absorb(h, out[-48:])
    beta, gamma = TR.challenge(h, 0), TR.challenge(h, 1)
    a, b = LO.lookup_columns([f], T_, m, beta)
    phi, last = LO.direct(a, b)
    assert last == 0, "the lookup does not hold"
    z, zlast = CO.z_of(c, beta, gamma)
    assert zlast == 1, "the copy constraints do not hold"
    out += com(z) + com(phi)
    h = TR.absorb(h, out[-96:])
    alpha = TR.challenge(h)
    T = quotient(lc, z, theta, beta, gamma, alpha, m, phi)
    tc = LN.chunks(T, n, log_ext)
    t48 = b"".join(g(PQ.horner(ch, secret)) for ch in tc)
    out += t48
    h = TR.absorb(h, t48)
    zeta = TR.challenge(h)
    r_l = linearisation(lc, z, T, log_ext, theta, beta, gamma, alpha, zeta, m, phi)
    assert PQ.horner(r_l, zeta) == 0
    polys, set_of, sets, ys = stack(lc, z, r_l, zeta, phi)
    evals = [y[0] for y in ys[1:]]
    ev = b"".join(TR.fr_bytes(x) for x in evals)
    out += ev
    h = TR.absorb(h, ev)
    v = TR.challenge(h)
    w = SO.proof_scalar(polys, set_of, sets, v, secret)
    out += g(w)
    assert len(out) == proof_size(t, log_ext, lc.c)
    assert challenges(n, t, log_ext, lc.c, c.ks, key48, public, out) == (theta, beta, gamma, alpha, zeta, v)
    return dict(proof=out, lc=lc, log_ext=log_ext, key48=key48, key_s=key_s, public=public, theta=theta, beta=beta, gamma=gamma,
                alpha=alpha, zeta=zeta, v=v, z=z, m=m, phi=phi, f=f, T=T, r_l=r_l, evals=evals, w=w)
