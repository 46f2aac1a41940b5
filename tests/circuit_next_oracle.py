"""Independent references for circuit proofs whose custom gates read the next row (kzg_circuit_create_custom_next ..
kzg_circuit_custom_next_verify_proof), in Python integers mod r, on top of circuit_custom_oracle and the
oracles under it.

A next-row circuit is a circuit_custom_oracle.CustomCircuit with a second exponent matrix p'[s][j] in 0..7; with i + 1 mod n

    every row:  sum_j q_j f_j + q_M f_0 f_1 + q_C + PI + sum_s qx_s[i] prod_j f_j[i]^p[s][j] prod_j f_j[i+1]^p'[s][j] = 0
    G'(X) = sum_s qx_s(X) prod_j f_j(X)^p[s][j] prod_j f_j(w X)^p'[s][j]         T = (Num + G') / (X^n - 1)
    r_N(X) = r(X) + sum_s (prod_j abar_j^p[s][j] prod_j abar'_j^p'[s][j]) qx_s(X),   abar'_j = f_j(zeta w), j in R

d_s = sum_j (p[s][j] + p'[s][j]), d_max = max d_s, R = { j : some p'[s][j] > 0 } ascending, rho = |R|.  f_j(w X) has the
coefficients of f_j with coefficient k scaled by w^k, so deg G' <= (d_max + 1)(n - 1) as in section 4.27, asserted wherever a
quotient is made.  Proofs are plain: there is no blinded next-row proof.

  * NextCircuit        the circuit, qx and both matrices; R, rho
  * shape_ok           the rules of kzg_circuit_create_custom_next
  * gprime_rows        G' on every row of H (row i + 1 mod n); gate_rows: the whole gate
  * shifted            f(w X) from f's coefficients
  * gprime_coeffs      G' as coefficients: products of values over a subgroup of more than deg G' points, one inverse transform
  * gprime_at          G'(zeta) from its definition, every polynomial by Horner, the next row at zeta w
  * quotient           T through circuit_oracle.quotient(extra = G'), the degrees asserted, padded as blind_oracle.quotient pads
  * remainder          the remainder of the numerator's division with changed wires, selectors or exponents
  * check_at           circuit_oracle.check_at with G'(zeta) from gprime_at
  * evaluations        (abar, sbar, zw, anext): anext the rho values f_j(zeta w), j in R
  * linearisation      r_N's coefficients
  * stack              the opening's (polys, set_of, sets, ys) on the three sets {zeta}, {zeta w}, {zeta, zeta w}
  * statement_hash, challenges, proof_size, layout, split   the transcript ("kzg_mi355x/plonk-custom-next/v1") and the format
  * prove              the proof bytes under a known secret (trapdoor_oracle's world)
"""
import hashlib

import blind_oracle as BO
import circuit_custom_oracle as CX
import circuit_oracle as CO
import linearise_oracle as LN
import ntt_oracle as NO
import open_sets_oracle as SO
import perm_quotient_oracle as PQ
import transcript_oracle as TR
import trapdoor_oracle as TO

R = PQ.R
DST = b"kzg_mi355x/plonk-custom-next/v1"
FIELDS = ("wires", "z", "chunks", "evals", "w")


class NextCircuit(CX.CustomCircuit):
    """circuit: a circuit_oracle.Circuit; q_custom: g columns of n integers; exps, exps_next: g rows of t integers in 0..7"""

    def __init__(self, circuit, q_custom, exps, exps_next):
        CX.CustomCircuit.__init__(self, circuit, q_custom, exps)
        self.exps_next = [list(row) for row in exps_next]
        assert len(self.exps_next) == self.g and all(len(row) == self.t for row in self.exps_next)
        self.d = [sum(a) + sum(b) for a, b in zip(self.exps, self.exps_next)]
        self.d_max = max(self.d)
        self.R = next_wires(self.exps_next)
        self.rho = len(self.R)

    def next_bytes(self):
        return bytes(p for row in self.exps_next for p in row)


def next_wires(exps_next):
    return [j for j in range(len(exps_next[0])) if any(row[j] for row in exps_next)]


def shape_ok(n, t, log_ext, exps, exps_next):
    """kzg_circuit_create_custom's rules with d_s over both matrices, rho >= 1 and n >= 2"""
    e, g = 1 << log_ext, len(exps)
    if not (1 <= g <= CX.MAX_CUSTOM) or len(exps_next) != g or n < 2:
        return False
    rows = [list(a) + list(b) for a, b in zip(exps, exps_next)]
    if any(len(row) != 2 * t or any(not 0 <= p <= 7 for p in row) or sum(row) < 1 for row in rows):
        return False
    if not next_wires(exps_next):
        return False
    return e >= max(t + 1, max(sum(row) for row in rows) + 1) and 3 * t + e + 3 + g <= CX.LIN_MAX_COLUMNS


def _term(row, row_next, f, f_next):
    return CX._monomial(row, f) * CX._monomial(row_next, f_next) % R


def gprime_rows(nc, wires=None, q_custom=None, exps=None, exps_next=None):
    f = nc.circuit.wires if wires is None else wires
    q = nc.q_custom if q_custom is None else q_custom
    ex = nc.exps if exps is None else exps
    en = nc.exps_next if exps_next is None else exps_next
    n = nc.n
    return [sum(q[s][i] * _term(ex[s], en[s], [col[i] for col in f], [col[(i + 1) % n] for col in f]) for s in range(nc.g)) % R
            for i in range(n)]


def gate_rows(nc, wires=None):
    return [(a + b) % R for a, b in zip(CO.gate_rows(nc.circuit, wires), gprime_rows(nc, wires))]


def shifted(coeffs, w):
    """f(w X): coefficient k times w^k"""
    out, p = [], 1
    for c in coeffs:
        out.append(c * p % R)
        p = p * w % R
    return out


def gprime_coeffs(nc, wire_coeffs=None, q_custom=None, exps=None, exps_next=None):
    """G' as coefficients (trailing zeros trimmed) from the wires' coefficient vectors (None: the circuit's wires, n each)"""
    wc = [NO.intt(list(col)) for col in nc.circuit.wires] if wire_coeffs is None else wire_coeffs
    q = nc.q_custom if q_custom is None else q_custom
    ex = nc.exps if exps is None else exps
    en = nc.exps_next if exps_next is None else exps_next
    n = nc.n
    w = NO.domain_root(NO.log2_exact(n))
    d_max = max(sum(a) + sum(b) for a, b in zip(ex, en))
    deg = (n - 1) + d_max * (max(len(c) for c in wc) - 1)
    M = 4
    while M <= deg or M < (d_max + 1) * n:
        M *= 2
    on = lambda cf: NO.ntt(list(cf) + [0] * (M - len(cf)))
    fv = [on(c) for c in wc]
    fn = [on(shifted(c, w)) for c in wc]
    qv = [on(NO.intt(list(col))) for col in q]
    vals = [sum(qv[s][i] * _term(ex[s], en[s], [col[i] for col in fv], [col[i] for col in fn]) for s in range(len(q))) % R
            for i in range(M)]
    g = PQ._trim(NO.intt(vals))
    assert len(g) <= deg + 1
    return g


def gprime_at(nc, wire_coeffs, zeta, key_coeffs=None):
    """G'(zeta) from its definition: every polynomial by Horner, the next row at zeta w"""
    w = NO.domain_root(NO.log2_exact(nc.n))
    f = [PQ.horner(c, zeta) for c in wire_coeffs]
    fn = [PQ.horner(c, zeta * w % R) for c in wire_coeffs]
    qs = [NO.intt(list(col)) for col in nc.q_custom] if key_coeffs is None else key_coeffs[2 * nc.t + 2:]
    return sum(PQ.horner(q, zeta) * _term(a, b, f, fn) for q, a, b in zip(qs, nc.exps, nc.exps_next)) % R


def coefficients(nc, z, log_ext):
    """(key: the 2 t + 2 + g columns, f, z, PI or None) as coefficient vectors of a plain proof, padded as blind_oracle pads"""
    return CX.coefficients(nc, z, BO.Blinders.zero(nc.t, log_ext))


def quotient(nc, z, log_ext, alpha, beta, gamma):
    """T padded to L_T coefficients (its first N - n are the plain call's), a zero remainder and the degrees asserted"""
    n, t, e = nc.n, nc.t, 1 << log_ext
    gp = gprime_coeffs(nc)
    assert len(gp) <= (nc.d_max + 1) * (n - 1) + 1
    T = PQ._trim(CO.quotient(nc.circuit, z, alpha, beta, gamma, extra=gp))
    assert len(T) <= max(t, nc.d_max) * n and len(T) <= (e - 1) * n
    LT = BO.quotient_len(n, t, log_ext)
    return T + [0] * (LT - len(T))


def remainder(nc, z, alpha, beta, gamma, wires=None, q_custom=None, exps=None, exps_next=None):
    wc = None if wires is None else [NO.intt(list(col)) for col in wires]
    return CO.remainder(nc.circuit, z, alpha, beta, gamma, wires, extra=gprime_coeffs(nc, wc, q_custom, exps, exps_next))


def check_at(zeta, T, nc, coefs, alpha, beta, gamma):
    key, wires, zc, pi = coefs
    return CO.check_at(zeta, T, nc.circuit, wires, zc, alpha, beta, gamma, extra=[gprime_at(nc, wires, zeta, key)],
                       key_coeffs=key[:2 * nc.t + 2], pi_coeffs=pi)


def evaluations(nc, coefs, zeta):
    abar, sbar, zw = BO.evaluations(nc.circuit, coefs, zeta)
    w = NO.domain_root(NO.log2_exact(nc.n))
    return list(abar), list(sbar), zw, [PQ.horner(coefs[1][j], zeta * w % R) for j in nc.R]


def next_terms(nc, abar, anext, exps=None, exps_next=None):
    """the g (scalar, ("key", 2 t + 2 + s)) that r_N has beyond r"""
    ex = nc.exps if exps is None else exps
    en = nc.exps_next if exps_next is None else exps_next
    full = [0] * nc.t
    for j, v in zip(nc.R, anext):
        full[j] = v
    return [(_term(ex[s], en[s], abar, full), ("key", 2 * nc.t + 2 + s)) for s in range(nc.g)]


def linearisation(nc, coefs, T, log_ext, alpha, beta, gamma, zeta, evals=None, exps=None, exps_next=None):
    """r_N's n + t + 3 coefficients (the tail is zero: the proof is plain)"""
    key, _, zc, _ = coefs
    c, n, t = nc.circuit, nc.n, nc.t
    bl = BO.Blinders.zero(t, log_ext)
    tc = BO.chunks(T, n, t, log_ext, bl)
    cols = {("z",): zc}
    cols.update({("key", j): key[j] for j in range(len(key))})
    cols.update({("T", k): tc[k] for k in range(len(tc))})
    abar, sbar, zw, anext = evaluations(nc, coefs, zeta) if evals is None else evals
    sc, const = LN.terms(c, coefs, log_ext, alpha, beta, gamma, zeta, evals=(abar, sbar, zw))
    sc = sc + next_terms(nc, abar, anext, exps, exps_next)
    r = [0] * (n + t + 3)
    for s, name in sc:
        for i, v in enumerate(cols[name]):
            r[i] = (r[i] + s * v) % R
    r[0] = (r[0] + const) % R
    return r


def stack(nc, coefs, r, zeta):
    """(polys, set_of, sets, ys): [ r_N | f_0 .. f_(t-1) | sigma_0 .. sigma_(t-2) | z ] on S_0 = {zeta}, S_1 = {zeta w},
    S_2 = {zeta, zeta w} (the wires of R, two values each)"""
    polys, set_of, sets, ys = BO.stack(nc.circuit, coefs, r, zeta)
    _, _, _, anext = evaluations(nc, coefs, zeta)
    set_of, ys = list(set_of), [list(y) for y in ys]
    for j, v in zip(nc.R, anext):
        set_of[1 + j] = 2
        ys[1 + j].append(v)
    return polys, set_of, sets + [[sets[0][0], sets[1][0]]], ys


def proof_size(t, log_ext, rho):
    return 48 * (t + (1 << log_ext) + 1) + 32 * (2 * t + rho)


def layout(t, log_ext, rho):
    e = 1 << log_ext
    sizes = (48 * t, 48, 48 * (e - 1), 32 * (2 * t + rho), 48)
    out, at = {}, 0
    for name, size in zip(FIELDS, sizes):
        out[name] = (at, at + size)
        at += size
    assert at == proof_size(t, log_ext, rho)
    return out


def split(proof, t, log_ext, rho):
    assert len(proof) == proof_size(t, log_ext, rho)
    return {name: proof[a:b] for name, (a, b) in layout(t, log_ext, rho).items()}


def statement_hash(n, t, log_ext, exps, exps_next, shifts, key48, public):
    g = len(exps)
    assert len(shifts) == t and len(key48) == 2 * t + 2 + g and all(len(k) == 48 for k in key48) and len(DST) == 31
    head = DST + b"".join(x.to_bytes(8, "big") for x in (n, t, log_ext, g, len(public)))
    return hashlib.sha256(head + b"".join(TR.fr_bytes(k) for k in shifts) + bytes(p for row in exps for p in row) +
                          bytes(p for row in exps_next for p in row) + b"".join(key48) +
                          b"".join(TR.fr_bytes(p) for p in public)).digest()


def challenges(n, t, log_ext, exps, exps_next, shifts, key48, public, proof):
    """(beta, gamma, alpha, zeta, v): transcript_oracle's chain from h1 on; v after all 2 t + rho evaluations"""
    f = split(proof, t, log_ext, len(next_wires(exps_next)))
    h = TR.absorb(statement_hash(n, t, log_ext, exps, exps_next, shifts, key48, public), f["wires"])
    beta, gamma = TR.challenge(h, 0), TR.challenge(h, 1)
    h = TR.absorb(h, f["z"])
    alpha = TR.challenge(h)
    h = TR.absorb(h, f["chunks"])
    zeta = TR.challenge(h)
    h = TR.absorb(h, f["evals"])
    return beta, gamma, alpha, zeta, TR.challenge(h)


def prove(oracle, nc, log_ext, secret, n_public=None):
    """The plain proof of the next-row circuit nc, mirroring circuit_custom_oracle.prove.  Returns a dict: proof (bytes), key48,
    public, the challenges and every intermediate"""
    c = nc.circuit
    n, t = c.n, c.t
    g = lambda s: TO.g1_scalar(oracle, s)
    public = TR.public_of(c, n_public)
    key_s = CX.key_scalars(nc, secret)
    key48 = [g(s) for s in key_s]
    h = statement_hash(n, t, log_ext, nc.exps, nc.exps_next, c.ks, key48, public)
    wires = [NO.intt(list(col)) for col in c.wires]
    wire_s = [PQ.horner(w, secret) for w in wires]
    out = b"".join(g(s) for s in wire_s)
    h = TR.absorb(h, out)
    beta, gamma = TR.challenge(h, 0), TR.challenge(h, 1)
    z, last = CO.z_of(c, beta, gamma)
    assert last == 1, "the copy constraints do not hold"
    coefs = coefficients(nc, z, log_ext)
    assert [w[:n] for w in coefs[1]] == wires and not any(x for w in coefs[1] for x in w[n:])
    z_s = PQ.horner(coefs[2], secret)
    out += g(z_s)
    h = TR.absorb(h, out[-48:])
    alpha = TR.challenge(h)
    T = quotient(nc, z, log_ext, alpha, beta, gamma)
    tc = BO.chunks(T, n, t, log_ext, BO.Blinders.zero(t, log_ext))
    t_s = [PQ.horner(ch, secret) for ch in tc]
    t48 = b"".join(g(s) for s in t_s)
    out += t48
    h = TR.absorb(h, t48)
    zeta = TR.challenge(h)
    abar, sbar, zw, anext = evaluations(nc, coefs, zeta)
    ev = b"".join(TR.fr_bytes(x) for x in abar + sbar + [zw] + anext)
    out += ev
    h = TR.absorb(h, ev)
    v = TR.challenge(h)
    r = linearisation(nc, coefs, T, log_ext, alpha, beta, gamma, zeta)
    assert PQ.horner(r, zeta) == 0
    polys, set_of, sets, ys = stack(nc, coefs, r, zeta)
    w = SO.proof_scalar(polys, set_of, sets, v, secret)
    out += g(w)
    assert len(out) == proof_size(t, log_ext, nc.rho)
    assert challenges(n, t, log_ext, nc.exps, nc.exps_next, c.ks, key48, public, out) == (beta, gamma, alpha, zeta, v)
    return dict(proof=out, nc=nc, log_ext=log_ext, key48=key48, key_s=key_s, public=public, beta=beta, gamma=gamma, alpha=alpha,
                zeta=zeta, v=v, z=z, coefs=coefs, T=T, chunks=tc, evals=(abar, sbar, zw, anext), r=r, wire_s=wire_s, z_s=z_s, t_s=t_s,
                w=w, stack=(polys, set_of, sets, ys))
