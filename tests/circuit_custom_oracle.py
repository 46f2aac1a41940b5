"""Independent references for circuit proofs with custom gates (kzg_circuit_create_custom .. kzg_circuit_custom_verify_proof;
DESIGN.md section 4.27), in Python integers mod r, on top of circuit_oracle, blind_oracle, linearise_oracle and transcript_oracle.

A custom circuit is a circuit_oracle.Circuit with g selector columns qx_s (n values each) and exponents p[s][j] in 0..7:

    every row:  sum_j q_j f_j + q_M f_0 f_1 + q_C + PI + sum_s qx_s prod_j f_j^p[s][j] = 0
    G'(X) = sum_s qx_s(X) prod_j f_j(X)^p[s][j]        Num_X = Num + G'        T = Num_X / (X^n - 1)
    r_X(X) = r(X) + sum_s (prod_j abar_j^p[s][j]) qx_s(X)

Degrees, asserted wherever a quotient is made: d_s = sum_j p[s][j], d_max = max d_s; deg G' <= (d_max + 1)(n - 1) and a plain T
has fewer than max(t, d_max) n coefficients; from blinded wires (n + 2 coefficients) deg G'~ <= n - 1 + d_max (n + 1) and
deg T~ = max(t n + t + 2, d_max (n + 1) - 1), exactly for n >= 4 and blinders that are all nonzero.

  * CustomCircuit      the circuit, qx and the exponents; key_columns(): circuit_oracle's, then qx[0..g)
  * shape_ok           the rules of kzg_circuit_create_custom; blinded_ok, blinded_keep: the blinded rule and deg T~ + 1
  * gprime_rows        G' on every row of H; gate_rows: the whole gate (all zero for a satisfied custom circuit)
  * gprime_coeffs      G' as coefficients from the wires' COEFFICIENTS (plain or blinded): products of values over a subgroup of more
                       than deg G' points (at least (d_max + 1) n), one inverse transform -- no coset, no division
  * gprime_at          G'(zeta) from its definition, every polynomial by Horner
  * coefficients       blind_oracle.coefficients with the qx_s behind the key (Blinders.zero: a plain proof's, zero-padded)
  * quotient           T (plain: through circuit_oracle.quotient(extra = G'); blinded: blind_oracle.numerator + G'~, divided), a zero
                       remainder and the degrees asserted, padded to L_T as blind_oracle.quotient pads
  * check_at           circuit_oracle.check_at with G'(zeta) from gprime_at
  * custom_terms       the g (scalar, ("key", 2 t + 2 + s)) of r_X; linearisation: r_X's coefficients
  * statement_hash, challenges   the transcript ("kzg_mi355x/plonk-custom/v1"); layout and split are transcript_oracle's
  * prove              the proof bytes under a known secret (trapdoor_oracle's world), mirroring transcript_oracle.prove
"""
import hashlib

import blind_oracle as BO
import circuit_oracle as CO
import linearise_oracle as LN
import ntt_oracle as NO
import open_sets_oracle as SO
import perm_quotient_oracle as PQ
import transcript_oracle as TR
import trapdoor_oracle as TO

R = PQ.R
DST = b"kzg_mi355x/plonk-custom/v1"
MAX_CUSTOM = 8
LIN_MAX_COLUMNS = 32


class CustomCircuit:
    """circuit: a circuit_oracle.Circuit; q_custom: g columns of n integers; exps: g rows of t integers in 0..7"""

    def __init__(self, circuit, q_custom, exps):
        self.circuit, self.q_custom, self.exps = circuit, [list(q) for q in q_custom], [list(row) for row in exps]
        self.n, self.t, self.g = circuit.n, circuit.t, len(q_custom)
        assert len(self.exps) == self.g and all(len(row) == self.t for row in self.exps)
        self.d = [sum(row) for row in self.exps]
        self.d_max = max(self.d)

    def key_columns(self):
        """the 2 t + 2 + g resident columns in the order of the key: circuit_oracle's, then qx[0..g)"""
        return self.circuit.key_columns() + self.q_custom

    def exps_bytes(self):
        return bytes(p for row in self.exps for p in row)


def shape_ok(t, log_ext, exps):
    """the rules of kzg_circuit_create_custom: 1 <= g <= 8, exponents in 0..7, every d_s >= 1, e >= max(t + 1, d_max + 1), and the
    plain proof's 3 t + e + 3 columns at zeta plus g within 32"""
    e, g = 1 << log_ext, len(exps)
    if not (1 <= g <= MAX_CUSTOM) or any(len(row) != t or any(not 0 <= p <= 7 for p in row) or sum(row) < 1 for row in exps):
        return False
    return e >= max(t + 1, max(sum(row) for row in exps) + 1) and 3 * t + e + 3 + g <= LIN_MAX_COLUMNS


def blinded_keep(n, t, d_max):
    """deg T~ + 1 = max(t n + t + 3, d_max (n + 1))"""
    return max(t * n + t + 3, d_max * (n + 1))


def blinded_ok(n, t, log_ext, d_max):
    """deg T~ + 1 <= L_T and N >= deg T~ + 2; for d_max <= t this is blind_oracle.shape_ok"""
    keep = blinded_keep(n, t, d_max)
    return BO.shape_ok(n, t, log_ext) and keep <= BO.quotient_len(n, t, log_ext) and (n << log_ext) >= keep + 1


def _monomial(row, f):
    v = 1
    for p, x in zip(row, f):
        v = v * pow(x, p, R) % R
    return v


def gprime_rows(cc, wires=None, q_custom=None, exps=None):
    f = cc.circuit.wires if wires is None else wires
    q = cc.q_custom if q_custom is None else q_custom
    ex = cc.exps if exps is None else exps
    return [sum(q[s][i] * _monomial(ex[s], [col[i] for col in f]) for s in range(cc.g)) % R for i in range(cc.n)]


def gate_rows(cc, wires=None):
    return [(a + b) % R for a, b in zip(CO.gate_rows(cc.circuit, wires), gprime_rows(cc, wires))]


def gprime_coeffs(cc, wire_coeffs=None, q_custom=None, exps=None):
    """G' as coefficients (trailing zeros trimmed) from the wires' coefficient vectors (None: the circuit's wires, n each)"""
    wc = [NO.intt(list(col)) for col in cc.circuit.wires] if wire_coeffs is None else wire_coeffs
    q = cc.q_custom if q_custom is None else q_custom
    ex = cc.exps if exps is None else exps
    n = cc.n
    d_max = max(sum(row) for row in ex)
    deg = (n - 1) + d_max * (max(len(w) for w in wc) - 1)
    M = 4
    while M <= deg or M < (d_max + 1) * n:
        M *= 2
    on = lambda cf: NO.ntt(list(cf) + [0] * (M - len(cf)))
    fv = [on(w) for w in wc]
    qv = [on(NO.intt(list(col))) for col in q]
    vals = [sum(qv[s][i] * _monomial(ex[s], [col[i] for col in fv]) for s in range(len(q))) % R for i in range(M)]
    g = PQ._trim(NO.intt(vals))
    assert len(g) <= deg + 1
    return g


def gprime_at(cc, wire_coeffs, zeta, key_coeffs=None):
    """G'(zeta) from its definition: every polynomial by Horner"""
    f = [PQ.horner(w, zeta) for w in wire_coeffs]
    qs = [NO.intt(list(col)) for col in cc.q_custom] if key_coeffs is None else key_coeffs[2 * cc.t + 2:]
    return sum(PQ.horner(q, zeta) * _monomial(row, f) for q, row in zip(qs, cc.exps)) % R


def coefficients(cc, z, bl):
    """(key: the 2 t + 2 + g columns, f~, z~, PI or None) as coefficient vectors; bl: blind_oracle.Blinders"""
    key, wires, zc, pi = BO.coefficients(cc.circuit, z, bl)
    return key + [NO.intt(list(col)) for col in cc.q_custom], wires, zc, pi


def _is_zero(bl):
    return not any(bl.flat())


def quotient(cc, coefs, log_ext, bl, alpha, beta, gamma, z=None):
    """T padded to L_T coefficients (as blind_oracle.quotient pads), a zero remainder and the degrees asserted.  With all blinders
    zero and z (values) given, the plain route: circuit_oracle.quotient(extra = G')"""
    c, n, t, e = cc.circuit, cc.n, cc.t, 1 << log_ext
    key, wires, zc, pi = coefs
    plain = _is_zero(bl)
    gp = gprime_coeffs(cc, [w[:n] for w in wires] if plain else wires)
    if plain:
        assert len(gp) <= (cc.d_max + 1) * (n - 1) + 1
        if z is not None:
            T = PQ._trim(CO.quotient(c, z, alpha, beta, gamma, extra=gp))
        else:
            T = None
    else:
        assert len(gp) <= n + cc.d_max * (n + 1)
        T = None
    if T is None:
        num = BO.numerator(c, (key[:2 * t + 2], wires, zc, pi), alpha, beta, gamma)
        m = max(len(num), len(gp))
        num = [(a + b) % R for a, b in zip(num + [0] * (m - len(num)), gp + [0] * (m - len(gp)))]
        T, rem = PQ.divide_vanishing(PQ._trim(num), n)
        assert rem == [], "Num_X is not divisible by X^n - 1"
        T = PQ._trim(T)
    LT = BO.quotient_len(n, t, log_ext)
    if plain:
        assert len(T) <= max(t, cc.d_max) * n and len(T) <= (e - 1) * n  # the custom share has degree below d_max n
    else:
        keep = blinded_keep(n, t, cc.d_max)
        assert len(T) <= keep
        if n >= 4 and all(bl.flat()[:2 * t + 3]):
            assert len(T) == keep, ("deg T~", len(T) - 1, keep - 1)
        assert blinded_ok(n, t, log_ext, cc.d_max), "the blinded rule refuses this shape"
    assert len(T) <= LT
    return T + [0] * (LT - len(T))


def remainder(cc, z, alpha, beta, gamma, wires=None, q_custom=None, exps=None):
    """the remainder of the plain numerator's division, with changed wires (values), selectors or exponents"""
    wc = None if wires is None else [NO.intt(list(col)) for col in wires]
    return CO.remainder(cc.circuit, z, alpha, beta, gamma, wires, extra=gprime_coeffs(cc, wc, q_custom, exps))


def check_at(zeta, T, cc, coefs, alpha, beta, gamma):
    """T(zeta) (zeta^n - 1) == Num(zeta) + G'(zeta): circuit_oracle.check_at with G' from its definition at zeta"""
    key, wires, zc, pi = coefs
    return CO.check_at(zeta, T, cc.circuit, wires, zc, alpha, beta, gamma, extra=[gprime_at(cc, wires, zeta, key)],
                       key_coeffs=key[:2 * cc.t + 2], pi_coeffs=pi)


def custom_terms(cc, abar, exps=None):
    ex = cc.exps if exps is None else exps
    return [(_monomial(ex[s], abar), ("key", 2 * cc.t + 2 + s)) for s in range(cc.g)]


def linearisation(cc, coefs, T, log_ext, bl, alpha, beta, gamma, zeta, evals=None, exps=None):
    """r_X's n + t + 3 coefficients (T: L_T coefficients; with Blinders.zero the tail is zero and the head is the plain r_X)"""
    key, _, zc, _ = coefs
    c, n, t = cc.circuit, cc.n, cc.t
    tc = BO.chunks(T, n, t, log_ext, bl)
    cols = {("z",): zc}
    cols.update({("key", j): key[j] for j in range(len(key))})
    cols.update({("T", k): tc[k] for k in range(len(tc))})
    abar = (BO.evaluations(c, coefs, zeta) if evals is None else evals)[0]
    sc, const = LN.terms(c, coefs, log_ext, alpha, beta, gamma, zeta, evals=evals)
    sc = sc + custom_terms(cc, abar, exps)
    r = [0] * (n + t + 3)
    for s, name in sc:
        for i, v in enumerate(cols[name]):
            r[i] = (r[i] + s * v) % R
    r[0] = (r[0] + const) % R
    return r


def statement_hash(n, t, log_ext, exps, shifts, key48, public):
    g = len(exps)
    assert len(shifts) == t and len(key48) == 2 * t + 2 + g and all(len(k) == 48 for k in key48)
    head = DST + b"".join(x.to_bytes(8, "big") for x in (n, t, log_ext, g, len(public)))
    assert len(DST) == 26
    return hashlib.sha256(head + b"".join(TR.fr_bytes(k) for k in shifts) + bytes(p for row in exps for p in row) + b"".join(key48) +
                          b"".join(TR.fr_bytes(p) for p in public)).digest()


def challenges(n, t, log_ext, exps, shifts, key48, public, proof):
    """(beta, gamma, alpha, zeta, v): transcript_oracle's chain from h1 on"""
    f = TR.split(proof, t, log_ext)
    h = TR.absorb(statement_hash(n, t, log_ext, exps, shifts, key48, public), f["wires"])
    beta, gamma = TR.challenge(h, 0), TR.challenge(h, 1)
    h = TR.absorb(h, f["z"])
    alpha = TR.challenge(h)
    h = TR.absorb(h, f["chunks"])
    zeta = TR.challenge(h)
    h = TR.absorb(h, f["evals"])
    return beta, gamma, alpha, zeta, TR.challenge(h)


def key_scalars(cc, secret):
    return [PQ.horner(NO.intt(list(col)), secret) for col in cc.key_columns()]


def prove(oracle, cc, log_ext, bl, secret, n_public=None):
    """The proof of the custom circuit cc under the blinders bl (BO.Blinders.zero: a plain proof), mirroring transcript_oracle.prove.
    Returns a dict: proof (bytes), key48, public, the challenges and every intermediate"""
    c = cc.circuit
    n, t = c.n, c.t
    g = lambda s: TO.g1_scalar(oracle, s)
    public = TR.public_of(c, n_public)
    key_s = key_scalars(cc, secret)
    key48 = [g(s) for s in key_s]
    h = statement_hash(n, t, log_ext, cc.exps, c.ks, key48, public)
    wires = [BO.blind(NO.intt(list(col)), b, n) for col, b in zip(c.wires, bl.b)]
    wire_s = [PQ.horner(w, secret) for w in wires]
    out = b"".join(g(s) for s in wire_s)
    h = TR.absorb(h, out)
    beta, gamma = TR.challenge(h, 0), TR.challenge(h, 1)
    z, last = CO.z_of(c, beta, gamma)
    assert last == 1, "the copy constraints do not hold"
    coefs = coefficients(cc, z, bl)
    assert coefs[1] == wires
    z_s = PQ.horner(coefs[2], secret)
    out += g(z_s)
    h = TR.absorb(h, out[-48:])
    alpha = TR.challenge(h)
    T = quotient(cc, coefs, log_ext, bl, alpha, beta, gamma, z=z)
    tc = BO.chunks(T, n, t, log_ext, bl)
    t_s = [PQ.horner(ch, secret) for ch in tc]
    t48 = b"".join(g(s) for s in t_s)
    out += t48
    h = TR.absorb(h, t48)
    zeta = TR.challenge(h)
    abar, sbar, zw = BO.evaluations(c, coefs, zeta)
    ev = b"".join(TR.fr_bytes(x) for x in list(abar) + list(sbar) + [zw])
    out += ev
    h = TR.absorb(h, ev)
    v = TR.challenge(h)
    r = linearisation(cc, coefs, T, log_ext, bl, alpha, beta, gamma, zeta)
    assert PQ.horner(r, zeta) == 0
    polys, set_of, sets, ys = BO.stack(c, coefs, r, zeta)
    w = SO.proof_scalar(polys, set_of, sets, v, secret)
    out += g(w)
    assert len(out) == TR.proof_size(t, log_ext)
    assert challenges(n, t, log_ext, cc.exps, c.ks, key48, public, out) == (beta, gamma, alpha, zeta, v)
    return dict(proof=out, cc=cc, log_ext=log_ext, key48=key48, key_s=key_s, public=public, beta=beta, gamma=gamma, alpha=alpha, zeta=zeta,
                v=v, z=z, coefs=coefs, T=T, chunks=tc, evals=(abar, sbar, zw), r=r, wire_s=wire_s, z_s=z_s, t_s=t_s, w=w)
