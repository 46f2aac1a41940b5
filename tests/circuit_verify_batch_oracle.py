"""Independent reference for the batch verifier of circuit proofs in the trapdoor world of
tests/transcript_oracle.py: every commitment of a proof is [c]G with a known scalar c, so the three G1 sums of the check

    e(P0, [1]G2) e(P1, [s]G2) e(P2, [s^2]G2) == 1

are [p0]G, [p1]G, [p2]G with scalars this module computes from the proof BYTES (the challenges are hashed from them, the
evaluations read from them) and the scalars of its points, and the pairing check is p0 + p1 s + p2 s^2 == 0 mod r.

For proof k with stack [r] | wires | sigma_0 .. sigma_(t-2) | [z], values 0 | abar | sbar | zw and weights v^i:
    A_0 = sum_(i < 2t) v^i C_i - sum_(i < 2t) v^i y_i        A_1 = v^(2t) ([z] - zw)
    p0 += rho (-zeta w A_0 - zeta A_1 - zeta^2 w W)
    p1 += rho (A_0 + A_1 + zeta (1 + w) W)
    p2 -= rho W
[r] comes from linearise_oracle.terms (the model of lin_scalars) and circuit_custom_oracle.custom_terms.

  * Member        one proof of a batch: its bytes, public inputs and the scalars of its t + e + 1 points
  * member        ... from transcript_oracle.prove's / circuit_custom_oracle.prove's dict
  * contribution  (a0, a1, w, zeta) of one proof: what does not depend on the weights
  * combine, sums (p0, p1, p2) of a batch under given weights
  * holds         p0 + p1 s + p2 s^2 == 0
  * points        the three sums as 48-byte compressed points"""
import circuit_custom_oracle as CX
import linearise_oracle as LN
import ntt_oracle as NO
import perm_quotient_oracle as PQ
import transcript_oracle as TR
import trapdoor_oracle as TO

R = PQ.R


class Member:
    def __init__(self, proof, public, wire_s, z_s, t_s, w):
        self.proof, self.public = bytes(proof), list(public)
        self.wire_s, self.z_s, self.t_s, self.w = list(wire_s), z_s, list(t_s), w


def member(d):
    return Member(d["proof"], d["public"], d["wire_s"], d["z_s"], d["t_s"], d["w"])


def evaluations(proof, t, log_ext):
    """(abar, sbar, zw) as the proof's bytes state them"""
    ev = TR.split(proof, t, log_ext)["evals"]
    vals = [int.from_bytes(ev[32 * i:32 * i + 32], "big") for i in range(2 * t)]
    assert all(v < R for v in vals)
    return vals[:t], vals[t:2 * t - 1], vals[2 * t - 1]


def public_input_at(n, public, zeta):
    """PI(zeta) by the barycentric rule, O(len(public)) where linearise_oracle's polynomial rule is O(n len(public)); the CPU test
    holds the two against each other"""
    w = NO.domain_root(NO.log2_exact(n))
    wi = [pow(w, i, R) for i in range(len(public))]
    if zeta % R in wi:
        return public[wi.index(zeta % R)] % R
    acc = sum(p * x % R * pow(zeta - x, -1, R) for p, x in zip(public, wi))
    return acc * (pow(zeta, n, R) - 1) % R * pow(n, -1, R) % R


def contribution(c, log_ext, key_s, key48, m, cc=None, challenges=None):
    """(a0, a1, w, zeta) of one proof: the scalars of A_0, A_1 and W, and its zeta.  c: the circuit (n, t, the shifts); cc: the custom
    circuit when the statement is the custom one (key_s, key48 then hold its 2 t + 2 + g entries); challenges: (beta, gamma, alpha,
    zeta, v) in the place of the hashed ones"""
    n, t = c.n, c.t
    if challenges is not None:
        beta, gamma, alpha, zeta, v = challenges
    elif cc is None:
        beta, gamma, alpha, zeta, v = TR.challenges(n, t, log_ext, c.ks, key48, m.public, m.proof)
    else:
        beta, gamma, alpha, zeta, v = CX.challenges(n, t, log_ext, cc.exps, c.ks, key48, m.public, m.proof)
    abar, sbar, zw = evaluations(m.proof, t, log_ext)
    sc, const = LN.terms(c, None, log_ext, alpha, beta, gamma, zeta, (abar, sbar, zw), public_input_at(n, m.public, zeta))
    if cc is not None:
        sc = sc + CX.custom_terms(cc, abar)
    at = {("z",): m.z_s}
    at.update({("key", j): key_s[j] for j in range(len(key_s))})
    at.update({("T", k): m.t_s[k] for k in range(len(m.t_s))})
    r_s = (sum(s * at[name] for s, name in sc) + const) % R
    stack = [r_s] + m.wire_s + [key_s[t + 2 + j] for j in range(t - 1)]
    ys = [0] + abar + sbar
    a0 = sum(pow(v, i, R) * (stack[i] - ys[i]) for i in range(2 * t)) % R
    a1 = pow(v, 2 * t, R) * (m.z_s - zw) % R
    return a0, a1, m.w % R, zeta


def combine(n, contributions, weights):
    """(p0, p1, p2) from the proofs' (a0, a1, w, zeta) and their weights"""
    w = NO.domain_root(NO.log2_exact(n))
    p0 = p1 = p2 = 0
    for (a0, a1, W, zeta), rho in zip(contributions, weights):
        p0 += rho * (-zeta * w % R * a0 - zeta * a1 - zeta * zeta % R * w % R * W)
        p1 += rho * (a0 + a1 + zeta * (1 + w) % R * W)
        p2 -= rho * W
    return p0 % R, p1 % R, p2 % R


def sums(c, log_ext, key_s, key48, members, weights, cc=None):
    return combine(c.n, [contribution(c, log_ext, key_s, key48, m, cc) for m in members], weights)


def holds(ps, s):
    return (ps[0] + ps[1] * s + ps[2] * s * s) % R == 0


def points(oracle, ps):
    return [TO.g1_scalar(oracle, p) for p in ps]
