"""CPU: kzg_circuit_proof_challenges and kzg_circuit_verify_proof on the circuits of
tests/circuit_edge_cases.py, against tests/transcript_oracle.py under a known secret (no GPU): public inputs on the first rows only
(0 < n_public < n, the statement n_public values long), and degenerate circuits whose proofs and keys carry points at infinity.

Shapes (n, t, log_ext): partial (8, 3, 2) with n_public 1, 3 and 7, (16, 2, 2) with 1, (16, 7, 3) with 2, and a column of zero
public inputs; every degenerate builder at (8, 3, 2), plain and blinded, and plain the idle circuit with one row, the zero witness
and the unused column at (16, 7, 3)."""
import pytest

import blind_oracle as BO
import circuit_edge_cases as EC
import kzg_poly_commit_exploration_amd as K
import test_circuit_proof as CP  # the known secret, its setup, _verify and _challenges
import transcript_oracle as TR

R = CP.R
srs = CP.srs
_CACHE = {}  # references computed once, shared and left unchanged


def _case(oracle, name, args, log_ext, blinded):
    key = (name, args, log_ext, blinded)
    if key not in _CACHE:
        c = EC.build(name, *args)
        bl = BO.Blinders.random(c.t, log_ext, 77 + c.n + c.t) if blinded else BO.Blinders.zero(c.t, log_ext)
        _CACHE[key] = EC.prove(oracle, c, log_ext, bl, CP.SECRET)
    return _CACHE[key]


def _oracle_challenges(d):
    return (d["beta"], d["gamma"], d["alpha"], d["zeta"], d["v"])


# ---- partial public inputs -------------------------------------------------------------------------------------------------------
PARTIAL = [("partial_public", (3, 3, 1, 11), 2), ("partial_public", (3, 3, 3, 12), 2), ("partial_public", (3, 3, 7, 13), 2),
           ("partial_public", (4, 2, 1, 14), 2), ("partial_public", (4, 7, 2, 15), 3), ("zero_public", (3, 3, 1), 2)]


@pytest.mark.parametrize("blinded", [True, False], ids=["blinded", "plain"])
@pytest.mark.parametrize("name,args,log_ext", PARTIAL)
def test_partial_public_inputs(oracle, srs, name, args, log_ext, blinded):
    d = _case(oracle, name, args, log_ext, blinded)
    c, public = d["c"], d["public"]
    n_public = args[2]
    assert len(public) == n_public and 0 < n_public < c.n and not any(c.pi[n_public:])
    assert all(public) == (name == "partial_public") and any(public) == (name == "partial_public")
    base = CP._challenges(oracle, d)
    assert base == _oracle_challenges(d) and len(set(base)) == 5
    assert CP._verify(oracle, srs, d)
    # the same proof under another statement.  A zero appended leaves the PI polynomial as it is: n_public alone tells them apart
    changed = list(public)
    changed[n_public - 1] = (changed[n_public - 1] + 1) % R
    others = [("padded with a zero", public + [0]), ("cut by one", public[:-1]), ("no public inputs", []), ("the last value changed", changed)]
    if n_public > 1:
        first = list(public)
        first[0] = (first[0] + 1) % R
        others.append(("the first value changed", first))
    for what, other in others:
        assert other != public
        assert CP._verify(oracle, srs, d, public=other) is False, what
    padded = CP._challenges(oracle, d, public=public + [0])
    assert all(a != b for a, b in zip(padded, base)), "a challenge does not depend on n_public"
    assert padded == TR.challenges(c.n, c.t, log_ext, c.ks, d["key48"], public + [0], d["proof"])


# ---- degenerate circuits ---------------------------------------------------------------------------------------------------------
SMALL = [("constant_witness", (3, 3, 0, 21)), ("constant_witness", (3, 3, EC.VALUE, 22)), ("idle", (3, 3)), ("zero_column", (3, 3, 23))]
DEGENERATE = [(name, args, 2, blinded) for name, args in SMALL for blinded in (False, True)] + \
             [("idle", (0, 3), 2, False), ("constant_witness", (4, 7, 0, 24), 3, False), ("zero_column", (4, 7, 25), 3, False)]
_ids = lambda cases: ["%s-%s-%s" % (c[0], "x".join(str(a)[:6] for a in c[1]), "blinded" if c[3] else "plain") for c in cases]


@pytest.mark.parametrize("name,args,log_ext,blinded", DEGENERATE, ids=_ids(DEGENERATE))
def test_degenerate_circuits(oracle, srs, name, args, log_ext, blinded):
    d = _case(oracle, name, args, log_ext, blinded)
    c, proof = d["c"], d["proof"]
    t = c.t
    assert CP._challenges(oracle, d) == _oracle_challenges(d)
    assert CP._verify(oracle, srs, d)
    # the points at infinity, read from the oracle's bytes, are where the builder says
    inf = EC.infinities(proof, t, log_ext)
    if blinded:
        assert inf == []
    else:
        want = EC.expected_infinities(name, args, t, log_ext)
        if want is not None:
            assert want and set(want) <= set(inf), (want, inf)
        if name == "constant_witness" and args[2] == 0:
            assert list(d["evals"][0]) == [0] * t
        if name == "zero_column":
            assert d["evals"][0][t - 1] == 0 and not any(d["coefs"][1][t - 1])
        if name == "idle":
            assert d["z"] == [1] * c.n and any(d["T"]) == (c.n == 1)
    # an infinity replaced by the generator, a finite point replaced by infinity: another proof, rejected
    generator = K.G1Point(oracle.p1_generator()).compress()
    assert generator != TR.INFINITY48 and len(generator) == 48
    for field in EC.POINT_FIELDS:
        a, b = TR.layout(t, log_ext)[field]
        for i in range((b - a) // 48):
            other = EC.replace_point(proof, t, log_ext, field, i, generator if (field, i) in inf else TR.INFINITY48)
            assert other != proof and len(other) == len(proof)
            assert CP._verify(oracle, srs, d, proof=other) is False, (field, i)
    # the key: idle's selector commitments are infinity
    key_inf = [j for j, k48 in enumerate(d["key48"]) if k48 == TR.INFINITY48]
    if name == "idle":
        assert key_inf == list(range(t + 2)) and d["key_s"][:t + 2] == [0] * (t + 2)
        for j in (0, t, t + 1):
            ks = list(d["key_s"])
            ks[j] = 1  # the generator
            assert CP._verify(oracle, srs, d, key_s=ks) is False, j
    else:
        assert key_inf == []
