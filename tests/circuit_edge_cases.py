"""Circuits that circuit_oracle.satisfied() never produces: public inputs on only the first rows, and
degenerate but legal circuits whose polynomials are zero or constant.  Builders only (not collected by pytest); each returns a
circuit_oracle.Circuit whose gate_rows() are all zero, with n_public set to what the statement carries (None: no public inputs).

  * partial_public    satisfied()'s circuit with public inputs on rows 0 .. n_public - 1 only, every one of them non-zero
  * zero_public       the same with a column of zeros: the statement carries n_public zero values, the PI polynomial is zero
  * constant_witness  satisfied()'s sigmas and selectors under a witness whose every cell is `value`
  * idle              nothing constrained: all selectors zero, the identity permutation, no public inputs
  * zero_column       a true permutation on columns 0 .. t - 2 and an unused last column of zeros

build(name, *args) calls a builder by name (the key of the tests' case caches), prove() is transcript_oracle.prove with the
circuit's n_public, and infinities() lists the point fields of a proof that are the point at infinity.  What a PLAIN proof of
each circuit holds at infinity is written with its builder; a blinded proof holds none anywhere."""
import random

import circuit_oracle as CO
import grand_product_oracle as GO
import transcript_oracle as TR

R = CO.R
POINT_FIELDS = ("wires", "z", "chunks", "w")


def _close(c, n_public):
    """q_const <- minus the gate's rows, so that every row holds"""
    c.q_const = [0] * c.n
    c.q_const = [(-v) % R for v in CO.gate_rows(c)]
    assert CO.gate_rows(c) == [0] * c.n
    c.n_public = n_public
    return c


def partial_public(k, t, n_public, seed):
    """Plain: no wire commitment, [z] or W is infinity (the last chunk is, where T is short: t = 2 with e = 4, or n = 2)"""
    c = CO.satisfied(k, t, seed, True)
    assert 0 < n_public < c.n
    rnd = random.Random(4100 + 17 * seed + n_public)
    c.pi = [rnd.randrange(1, R) if i < n_public else 0 for i in range(c.n)]
    return _close(c, n_public)


def zero_public(k, t, n_public, seed=0):
    """Plain: no field is infinity.  PI = 0, yet n_public and the zeros are part of the statement"""
    c = CO.satisfied(k, t, seed, True)
    assert 0 < n_public < c.n
    c.pi = [0] * c.n
    return _close(c, n_public)


def constant_witness(k, t, value, seed):
    """Any permutation holds for this witness.  Public inputs on all n rows, as satisfied() gives them.
    Plain, value = 0: all t wire commitments are infinity and all wire evaluations are zero.
    Plain, value != 0: every wire polynomial is the constant `value`; no field is infinity"""
    c = CO.satisfied(k, t, seed, True)
    c.wires = [[value % R] * c.n for _ in range(t)]
    return _close(c, c.n)


def idle(k, t):
    """z = 1, and of the key every commitment but the sigmas' is infinity.  At n > 1 T = 0: plain, all e - 1 chunk commitments
    are infinity.  At n = 1 sigma_j = k_j is not the polynomial k_j X, so T is not zero and the chunks are finite; plain, it is
    the opening proof W that is infinity there"""
    n = 1 << k
    ks = GO.shifts(t)
    rnd = random.Random(4300 + 5 * k + t)
    wires = [[rnd.randrange(R) for _ in range(n)] for _ in range(t)]
    zeros = lambda: [0] * n
    return _close(CO.Circuit(ks, wires, GO.identity_sigmas(k, ks), [zeros() for _ in range(t)], zeros(), zeros(), None), None)


def zero_column(k, t, seed):
    """Column t - 1 is unused: zeros under the identity permutation.  Two public inputs.
    Plain: wire commitment t - 1 is infinity and abar[t - 1] = 0 (at t = 3, e = 4 the last chunk too: T is a column shorter)"""
    assert t >= 3 and k >= 2
    n = 1 << k
    ks = GO.shifts(t)
    wires, sigmas = GO.true_permutation(k, t - 1, ks[:t - 1], seed)
    wires.append([0] * n)
    sigmas.append(GO.identity_sigmas(k, ks)[t - 1])
    rnd = random.Random(4500 + 31 * seed + t)
    q_lin = [[rnd.randrange(R) for _ in range(n)] for _ in range(t)]
    q_mul = [rnd.randrange(R) for _ in range(n)]
    pi = [rnd.randrange(1, R) if i < 2 else 0 for i in range(n)]
    return _close(CO.Circuit(ks, wires, sigmas, q_lin, q_mul, [0] * n, pi), 2)


BUILDERS = dict(partial_public=partial_public, zero_public=zero_public, constant_witness=constant_witness, idle=idle,
                zero_column=zero_column)
VALUE = 0x1F2E3D4C5B6A79788796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF % R  # constant_witness's non-zero value


def build(name, *args):
    return BUILDERS[name](*args)


def prove(oracle, c, log_ext, bl, secret):
    """transcript_oracle.prove under the statement the builder meant"""
    return TR.prove(oracle, c, log_ext, bl, secret, n_public=c.n_public)


def infinities(proof, t, log_ext):
    """[(field, index)] of the points of `proof` that are the point at infinity, read from the bytes"""
    f = TR.split(proof, t, log_ext)
    return [(name, i) for name in POINT_FIELDS for i in range(len(f[name]) // 48) if f[name][48 * i:48 * i + 48] == TR.INFINITY48]


def expected_infinities(name, args, t, log_ext):
    """the fields a PLAIN proof of the case must hold at infinity (the point of the case; more may be: a short T's last chunk);
    None where none has to be"""
    e = 1 << log_ext
    if name == "constant_witness" and args[2] == 0:
        return [("wires", j) for j in range(t)]
    if name == "idle":
        return [("w", 0)] if args[0] == 0 else [("chunks", i) for i in range(e - 1)]
    if name == "zero_column":
        return [("wires", t - 1)]
    return None


def replace_point(proof, t, log_ext, field, index, data):
    a = TR.layout(t, log_ext)[field][0] + 48 * index
    return proof[:a] + data + proof[a + 48:]
