"""Independent reference for a circuit's proof as bytes: the hashed transcript with hashlib, chained round
by round over blind_oracle / circuit_oracle / linearise_oracle under a known secret (trapdoor_oracle's world: every commitment is
[P(s)]G, one scalar multiplication of the generator by the C oracle).

    DST = b"kzg_mi355x/plonk/v1"
    h0  = SHA256(DST | u64be(n) | u64be(t) | u64be(log_ext) | u64be(n_public) | shifts | key commitments | public inputs)
    h1  = SHA256(h0 | wire commitments)       beta = fr(SHA256(h1 | 00)), gamma = fr(SHA256(h1 | 01))
    h2  = SHA256(h1 | [z])                    alpha = fr(SHA256(h2 | 00))
    h3  = SHA256(h2 | [T_0] .. [T_(e-2)])     zeta = fr(SHA256(h3 | 00))
    h4  = SHA256(h3 | evaluations)            v = fr(SHA256(h4 | 00))

scalars as 32 big-endian bytes, points as 48 compressed bytes, fr(d) = int(d, big-endian) mod r.  A proof is the wire commitments,
[z], the chunk commitments, the 2 t evaluations (abar, sbar, z(zeta w)) and W, in that order.

  * statement_hash, absorb, challenge   the pieces of the chain
  * challenges                          (beta, gamma, alpha, zeta, v) from complete proof bytes
  * layout, split                       the byte ranges of the five fields; the fields of a proof
  * prove                               the proof of a satisfied circuit: the wires' scalars -> beta, gamma -> z -> alpha -> T ->
                                        zeta -> the evaluations -> v -> W; with every intermediate the tests compare against
A plain proof is the blinded chain with all blinders zero (tests/test_circuit_blinded_gpu.py holds the library to that)."""
import hashlib

import blind_oracle as BO
import circuit_oracle as CO
import ntt_oracle as NO
import open_sets_oracle as SO
import perm_quotient_oracle as PQ
import trapdoor_oracle as TO

R = PQ.R
DST = b"kzg_mi355x/plonk/v1"
FIELDS = ("wires", "z", "chunks", "evals", "w")
INFINITY48 = b"\xc0" + bytes(47)


def fr_bytes(v):
    return (v % R).to_bytes(32, "big")


def challenge(h, tag=0):
    return int.from_bytes(hashlib.sha256(h + bytes([tag])).digest(), "big") % R


def absorb(h, data):
    return hashlib.sha256(h + data).digest()


def statement_hash(n, t, log_ext, shifts, key48, public):
    assert len(shifts) == t and len(key48) == 2 * t + 2 and all(len(k) == 48 for k in key48)
    head = DST + b"".join(x.to_bytes(8, "big") for x in (n, t, log_ext, len(public)))
    return hashlib.sha256(head + b"".join(fr_bytes(k) for k in shifts) + b"".join(key48) + b"".join(fr_bytes(p) for p in public)).digest()


def proof_size(t, log_ext):
    return 48 * (t + (1 << log_ext) + 1) + 64 * t


def layout(t, log_ext):
    """{field: (first byte, end)}"""
    e = 1 << log_ext
    sizes = (48 * t, 48, 48 * (e - 1), 64 * t, 48)
    out, at = {}, 0
    for name, size in zip(FIELDS, sizes):
        out[name] = (at, at + size)
        at += size
    assert at == proof_size(t, log_ext)
    return out


def split(proof, t, log_ext):
    assert len(proof) == proof_size(t, log_ext)
    return {name: proof[a:b] for name, (a, b) in layout(t, log_ext).items()}


def challenges(n, t, log_ext, shifts, key48, public, proof):
    """(beta, gamma, alpha, zeta, v): the bytes are hashed as they are"""
    f = split(proof, t, log_ext)
    h = absorb(statement_hash(n, t, log_ext, shifts, key48, public), f["wires"])
    beta, gamma = challenge(h, 0), challenge(h, 1)
    h = absorb(h, f["z"])
    alpha = challenge(h)
    h = absorb(h, f["chunks"])
    zeta = challenge(h)
    h = absorb(h, f["evals"])
    return beta, gamma, alpha, zeta, challenge(h)


def public_of(c, n_public=None):
    """the statement's public inputs: rows 0 .. n_public - 1 of the circuit's column (all n when not given), the rest zero"""
    if c.pi is None:
        assert not n_public
        return []
    n_public = c.n if n_public is None else n_public
    assert not any(c.pi[n_public:]), "a public input beyond n_public"
    return list(c.pi[:n_public])


def key_scalars(c, secret):
    return [PQ.horner(NO.intt(col), secret) for col in c.key_columns()]


def prove(oracle, c, log_ext, bl, secret, n_public=None):
    """The proof of circuit c under the blinders bl (BO.Blinders.zero: a plain proof).  Returns a dict: proof (bytes), key48, public,
    the challenges, z (values), coefs, T, chunks, evals, and the scalars wire_s, z_s, t_s, w of the commitments."""
    n, t = c.n, c.t
    g = lambda s: TO.g1_scalar(oracle, s)
    public = public_of(c, n_public)
    key_s = key_scalars(c, secret)
    key48 = [g(s) for s in key_s]
    h = statement_hash(n, t, log_ext, c.ks, key48, public)
    # round 1: the wires
    wires = [BO.blind(NO.intt(col), b, n) for col, b in zip(c.wires, bl.b)]
    wire_s = [PQ.horner(w, secret) for w in wires]
    out = b"".join(g(s) for s in wire_s)
    h = absorb(h, out)
    beta, gamma = challenge(h, 0), challenge(h, 1)
    # round 2: z
    z, last = CO.z_of(c, beta, gamma)
    assert last == 1, "the copy constraints do not hold"
    coefs = BO.coefficients(c, z, bl)
    assert coefs[1] == wires
    z_s = PQ.horner(coefs[2], secret)
    out += g(z_s)
    h = absorb(h, out[-48:])
    alpha = challenge(h)
    # round 3: the quotient's chunks
    T = BO.quotient(c, coefs, log_ext, alpha, beta, gamma)
    tc = BO.chunks(T, n, t, log_ext, bl)
    t_s = [PQ.horner(ch, secret) for ch in tc]
    t48 = b"".join(g(s) for s in t_s)
    out += t48
    h = absorb(h, t48)
    zeta = challenge(h)
    # round 4: the evaluations
    abar, sbar, zw = BO.evaluations(c, coefs, zeta)
    ev = b"".join(fr_bytes(x) for x in list(abar) + list(sbar) + [zw])
    out += ev
    h = absorb(h, ev)
    v = challenge(h)
    # round 5: the opening
    r = BO.linearisation(c, coefs, T, log_ext, bl, alpha, beta, gamma, zeta)
    assert PQ.horner(r, zeta) == 0
    polys, set_of, sets, ys = BO.stack(c, coefs, r, zeta)
    w = SO.proof_scalar(polys, set_of, sets, v, secret)
    out += g(w)
    assert len(out) == proof_size(t, log_ext)
    assert challenges(n, t, log_ext, c.ks, key48, public, out) == (beta, gamma, alpha, zeta, v)
    return dict(proof=out, c=c, log_ext=log_ext, key48=key48, key_s=key_s, public=public, beta=beta, gamma=gamma, alpha=alpha, zeta=zeta,
                v=v, z=z, coefs=coefs, T=T, chunks=tc, evals=(abar, sbar, zw), wire_s=wire_s, z_s=z_s, t_s=t_s, w=w)
