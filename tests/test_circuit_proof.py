"""CPU: a circuit's proof as bytes -- kzg_circuit_proof_size, kzg_circuit_proof_challenges and
kzg_circuit_verify_proof against tests/transcript_oracle.py (hashlib, the big-integer oracles, commitments from the known secret:
no GPU).

Shapes (n, t, log_ext): (8, 3, 2) the smallest blinded shape with e = t + 1, (16, 2, 2) with e > t + 1 (a plain proof's last chunk
is zero and travels as the point at infinity), (16, 7, 3) the widest circuit, and (1, 3, 2) plain: one row."""
import ctypes as C

import numpy as np
import pytest

import blind_oracle as BO
import circuit_oracle as CO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import perm_quotient_oracle as PQ
import transcript_oracle as TR
import trapdoor_oracle as TO

R = PQ.R
SECRET = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % R
SHAPES = [(8, 3, 2), (16, 2, 2), (16, 7, 3)]
INV = K.KZG_ERR_INVALID_ARG
_CACHE = {}  # references computed once, shared and left unchanged


def _case(oracle, n, t, log_ext, with_pi=True, blinded=True, seed=0):
    key = (n, t, log_ext, with_pi, blinded, seed)
    if key not in _CACHE:
        c = CO.satisfied(NO.log2_exact(n), t, 500 + n + t, with_pi)
        bl = BO.Blinders.random(t, log_ext, 10 * seed + n + t) if blinded else BO.Blinders.zero(t, log_ext)
        _CACHE[key] = TR.prove(oracle, c, log_ext, bl, SECRET)
    return _CACHE[key]


@pytest.fixture(scope="module")
def srs(oracle):
    """[s^j]G1 for j < 2 and [s^j]G2 for j <= 2"""
    g1 = np.stack([oracle.p1_mult(oracle.p1_generator(), pow(SECRET, j, R)) for j in range(2)])
    g2 = np.stack([K.srs_g2_at(TO.secret_be(SECRET), j) for j in range(3)])
    return g1, g2


def _key(oracle, d, key_s=None):
    return [K.G1Point(oracle.p1_mult(oracle.p1_generator(), s % R)) for s in (d["key_s"] if key_s is None else key_s)]


def _scalars(values):
    return [K.Scalar(x) for x in values]


def _challenges(oracle, d, proof=None, key_s=None, shifts=None, public=None):
    c = d["c"]
    got = K.circuit_proof_challenges(_key(oracle, d, key_s), c.n, d["log_ext"], _scalars(c.ks if shifts is None else shifts),
                                     _scalars(d["public"] if public is None else public), d["proof"] if proof is None else proof)
    return tuple(x.v for x in got)


def _verify(oracle, srs, d, proof=None, key_s=None, public=None):
    c = d["c"]
    return K.circuit_verify_proof(_key(oracle, d, key_s), c.n, d["log_ext"], _scalars(c.ks), _scalars(d["public"] if public is None else public),
                                  d["proof"] if proof is None else proof, srs[0], srs[1])


def _flip(proof, at, bit=1):
    b = bytearray(proof)
    b[at] ^= bit
    return bytes(b)


# ---- the format ------------------------------------------------------------------------------------------------------------------
def test_proof_size_against_the_formula():
    lib = K.load_library()
    for log_ext in range(0, 5):
        for t in range(0, 10):
            legal = 2 <= t <= K.KZG_PQ_MAX_COLUMNS and log_ext <= K.KZG_PQ_MAX_LOG_EXT and t + 1 <= 1 << log_ext
            out = C.c_size_t(12345)
            rc = lib.kzg_circuit_proof_size(t, log_ext, C.byref(out))
            if legal:
                assert rc == 0 and out.value == 48 * (t + (1 << log_ext) + 1) + 64 * t == TR.proof_size(t, log_ext), (t, log_ext)
            else:
                assert rc == INV and out.value == 12345, (t, log_ext)
    assert K.circuit_proof_size(3, 2) == 576
    assert lib.kzg_circuit_proof_size(3, 2, None) == INV


# ---- the transcript --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blinded", [True, False], ids=["blinded", "plain"])
@pytest.mark.parametrize("with_pi", [True, False], ids=["pi", "no_pi"])
@pytest.mark.parametrize("n,t,log_ext", SHAPES)
def test_challenges_against_the_oracle(oracle, n, t, log_ext, with_pi, blinded):
    d = _case(oracle, n, t, log_ext, with_pi, blinded)
    assert len(d["public"]) == (n if with_pi else 0)
    assert _challenges(oracle, d) == (d["beta"], d["gamma"], d["alpha"], d["zeta"], d["v"])
    assert len(set(_challenges(oracle, d))) == 5


@pytest.mark.parametrize("n,t,log_ext", SHAPES)
def test_every_input_changes_the_challenges_after_it_and_none_before(oracle, n, t, log_ext):
    d = _case(oracle, n, t, log_ext)
    c, base = d["c"], _challenges(oracle, d)

    def changed(got, first):
        """the challenges from index `first` on differ (beta, gamma, alpha, zeta, v), the earlier ones do not"""
        assert got[:first] == base[:first], (first, "an earlier challenge moved")
        assert all(a != b for a, b in zip(got[first:], base[first:])), (first, "a later challenge stayed")

    # the statement: everything moves
    for j in (0, t + 1, 2 * t + 1):
        ks = list(d["key_s"])
        ks[j] = (ks[j] + 1) % R
        changed(_challenges(oracle, d, key_s=ks), 0)
    for j in (0, t - 1):
        sh = list(c.ks)
        sh[j] = (sh[j] + 1) % R
        changed(_challenges(oracle, d, shifts=sh), 0)
    pub = list(d["public"])
    pub[-1] = (pub[-1] + 1) % R
    changed(_challenges(oracle, d, public=pub), 0)
    changed(_challenges(oracle, d, public=d["public"] + [0] if len(d["public"]) < n else d["public"][:-1]), 0)  # n_public alone
    # one byte of each proof field: the first and the last byte of the field
    first = {"wires": 0, "z": 2, "chunks": 3, "evals": 4, "w": 5}
    for name, (a, b) in TR.layout(t, log_ext).items():
        for at in (a, b - 1):
            changed(_challenges(oracle, d, proof=_flip(d["proof"], at, 0x04)), first[name])


# ---- the verifier ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blinded", [True, False], ids=["blinded", "plain"])
@pytest.mark.parametrize("n,t,log_ext", SHAPES)
def test_verifier_accepts_and_rejects(oracle, srs, n, t, log_ext, blinded):
    d = _case(oracle, n, t, log_ext, True, blinded)
    assert _verify(oracle, srs, d)
    assert _verify(oracle, srs, _case(oracle, n, t, log_ext, False, blinded))  # without public inputs
    proof = d["proof"]
    L = TR.layout(t, log_ext)
    # a byte of each field.  Points: the last byte of the abscissa (most such points are off the curve: valid = 0 either way);
    # evaluations: the last byte, still below r
    for name, (a, b) in L.items():
        assert not _verify(oracle, srs, d, proof=_flip(proof, b - 1)), name
    # the sign bit of a point: another point of the curve
    for name in ("wires", "z", "chunks", "w"):
        a = L[name][0]
        if proof[a:a + 48] != TR.INFINITY48:
            assert not _verify(oracle, srs, d, proof=_flip(proof, a, 0x20)), name
    # two wire commitments swapped
    swapped = proof[48:96] + proof[:48] + proof[96:]
    assert swapped != proof and not _verify(oracle, srs, d, proof=swapped)
    # the statement
    pub = list(d["public"])
    pub[0] = (pub[0] + 1) % R
    assert not _verify(oracle, srs, d, public=pub)
    ks = list(d["key_s"])
    ks[t] = (ks[t] + 1) % R
    assert not _verify(oracle, srs, d, key_s=ks)


def test_one_row_plain(oracle, srs):
    d = _case(oracle, 1, 3, 2, True, False)
    assert _verify(oracle, srs, d)
    assert not _verify(oracle, srs, d, proof=_flip(d["proof"], TR.layout(3, 2)["evals"][1] - 1))


@pytest.mark.parametrize("n", [16, 2])
def test_a_zero_chunk_travels_as_infinity(oracle, srs, n):
    """plain, t = 2, e = 4: T has at most 2 n coefficients, so the third chunk is zero"""
    d = _case(oracle, n, 2, 2, True, False)
    assert not any(d["chunks"][2]) and d["t_s"][2] == 0 and any(d["chunks"][0])
    a = TR.layout(2, 2)["chunks"][0]
    assert d["proof"][a + 96:a + 144] == TR.INFINITY48
    assert _verify(oracle, srs, d)


def test_bytes_that_do_not_decode_are_invalid_not_errors(oracle, srs):
    n, t, log_ext = 8, 3, 2
    d = _case(oracle, n, t, log_ext)
    proof, L = d["proof"], TR.layout(t, log_ext)

    def put(at, data):
        return proof[:at] + data + proof[at + len(data):]

    a = L["evals"][0]
    canonical = int.from_bytes(proof[a:a + 32], "big")
    assert canonical + R < 1 << 256
    bad = [("an evaluation plus r", put(a, (canonical + R).to_bytes(32, "big"))),
           ("an evaluation equal to r", put(L["evals"][1] - 32, R.to_bytes(32, "big")))]
    # an abscissa with no point: walk the last byte until the verifier's decoder refuses it
    lib = K.load_library()
    out = np.zeros(18, dtype=np.uint64)
    for field in ("wires", "z", "chunks", "w"):
        at = L[field][0]
        for delta in range(1, 64):
            cand = bytearray(proof[at:at + 48])
            cand[47] = (cand[47] + delta) & 0xFF
            if lib.kzg_g1_uncompress(bytes(cand), out.ctypes.data_as(C.c_void_p)) != 0:
                bad.append((field + " off the curve", put(at, bytes(cand))))
                break
        else:
            raise AssertionError("no abscissa off the curve near " + field)
    # flag bits: no compression flag; infinity flag with an abscissa; infinity with the sign bit
    w = L["w"][0]
    bad.append(("uncompressed flag", _flip(proof, w, 0x80)))
    bad.append(("infinity flag on a finite point", _flip(proof, w, 0x40)))
    bad.append(("infinity with a sign", put(L["z"][0], b"\xe0" + bytes(47))))
    bad.append(("abscissa not below p", put(w, b"\x9f" + b"\xff" * 47)))
    for what, data in bad:
        assert len(data) == len(proof)
        assert _verify(oracle, srs, d, proof=data) is False, what  # KZG_OK (no exception), valid = 0


def test_argument_errors(oracle, srs):
    lib = K.load_library()
    n, t, log_ext = 8, 3, 2
    d = _case(oracle, n, t, log_ext)
    c = d["c"]
    key = np.ascontiguousarray(np.stack([p.p1 for p in _key(oracle, d)]), dtype=np.uint64)
    ks = np.ascontiguousarray(np.stack([K.Scalar(k).limbs() for k in c.ks]))
    pub = np.ascontiguousarray(np.stack([K.Scalar(p).limbs() for p in d["public"]]))
    buf = np.frombuffer(d["proof"], dtype=np.uint8).copy()
    g1, g2 = np.ascontiguousarray(srs[0]), np.ascontiguousarray(srs[1])
    out = np.zeros((5, 4), dtype=np.uint64)
    ok = C.c_int(7)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def challenges(key=key, n=n, t=t, log_ext=log_ext, ks=ks, pub=pub, n_public=n, buf=buf, length=len(buf), out=out):
        return lib.kzg_circuit_proof_challenges(p(key), n, t, log_ext, p(ks), p(pub), n_public, p(buf), length, p(out))

    def verify(key=key, n=n, t=t, log_ext=log_ext, ks=ks, pub=pub, n_public=n, buf=buf, length=len(buf), g1=g1, g2=g2, valid=ok):
        return lib.kzg_circuit_verify_proof(p(key), n, t, log_ext, p(ks), p(pub), n_public, p(buf), length, p(g1), 144, p(g2), 288,
                                            None if valid is None else C.byref(valid))

    assert challenges() == 0 and verify() == 0 and ok.value == 1
    ok.value = 7
    not_fr = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    bad_ks, bad_pub = ks.copy(), pub.copy()
    bad_ks[t - 1] = not_fr
    bad_pub[n - 1] = not_fr
    for call in (challenges, verify):
        for name in ("key", "ks", "pub", "buf"):
            assert call(**{name: None}) == INV, name
        assert call(pub=None, n_public=0) == 0  # no public inputs: the pointer may be NULL
        for length in (0, len(buf) - 1, len(buf) + 1, TR.proof_size(2, 2)):
            assert call(length=length) == INV, length
        assert call(n=12) == INV and call(n=0) == INV and call(n=1 << 23) == INV
        assert call(t=1) == INV and call(t=8) == INV and call(t=4) == INV  # t + 1 > e
        assert call(log_ext=4) == INV
        assert call(n_public=n + 1) == INV
        assert call(ks=bad_ks) == INV and call(pub=bad_pub) == INV
    assert challenges(out=None) == INV
    assert verify(g1=None) == INV and verify(g2=None) == INV and verify(valid=None) == INV
    assert ok.value in (0, 7)  # (the call without public inputs is a false statement: valid = 0)
    # a key commitment off the curve: kzg_circuit_verify's error, after a proof that decodes
    off = key.copy()
    off[1, 0] ^= np.uint64(1)
    assert verify(key=off) == INV


def test_header_wrapper_and_library_agree():
    lib = K.load_library()
    header = open(K.__file__.replace("kzg_poly_commit_exploration_amd/__init__.py", "include/kzg_mi355x.h")).read()
    for name in ("kzg_circuit_proof_size", "kzg_circuit_proof_challenges", "kzg_circuit_verify_proof"):
        assert "int %s(" % name in header and name in K.ABI_SYMBOLS and hasattr(lib, name)
        assert name[4:] in K.__all__ and callable(getattr(K, name[4:]))
