"""CPU: the interface of the batch verifier of circuit proofs is declared where the other calls are, and
the reference the GPU test compares against (tests/circuit_verify_batch_oracle.py) is itself checked: in the trapdoor world the
pairing product e(P0, [1]G2) e(P1, [s]G2) e(P2, [s^2]G2) is [p0 + p1 s + p2 s^2] of the target group's generator, so the model's
three scalars must satisfy p0 + p1 s + p2 s^2 == 0 exactly when every proof of the batch is one the per-proof verifier accepts.
(oracle/pairing_twin.py is not needed for that: the check runs in the exponent.)

The three test_the_model* tests exercise the test oracle alone, not the library: they pass on any commit that has the oracle
modules they import, and show nothing about the feature.  They are here so that the reference the GPU test trusts is checked
without a GPU.  The other tests read the header, the wrapper lists and the new unit's source, and fail without the feature."""
import os
import re

import circuit_custom_cases as CC
import circuit_custom_oracle as CX
import circuit_proof_cases as CP
import circuit_verify_batch_oracle as VB
import kzg_poly_commit_exploration_amd as K
import transcript_oracle as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = VB.R
NAMES = ("kzg_circuit_verify_proofs_batch", "kzg_circuit_verify_proofs_lincomb", "kzg_circuit_verify_proofs_lincomb_challenges")


def _header():
    with open(os.path.join(ROOT, "include", "kzg_mi355x.h")) as f:
        return f.read()


def test_the_header_and_the_wrapper_lists_carry_both_symbols_and_the_cap():
    text = _header()
    for name in NAMES:
        assert re.search(r"\bint %s\(kzg_ctx\* ctx," % name, text), name
        assert name in K.ABI_SYMBOLS
    assert re.search(r"#define KZG_VERIFY_MAX_PROOFS \(1u << 16\)", text) and K.KZG_VERIFY_MAX_PROOFS == 1 << 16
    assert "KZG_ABI_VERSION 4" in text and K.KZG_ABI_VERSION == 4
    assert hasattr(K.Engine, "circuit_verify_proofs_batch") and hasattr(K.Engine, "circuit_verify_proofs_lincomb")
    with open(os.path.join(ROOT, "kzg_poly_commit_exploration_amd", "__init__.py")) as f:
        table = f.read()
    for name in NAMES:  # the ctypes table
        assert re.search(r'"%s": \(i, \[' % name, table), name


def test_the_header_documents_the_status_order_and_what_is_not_offered():
    text = _header()
    at = text.index("kzg_circuit_verify_proofs_batch: proof k")
    doc = text[at:text.index("#define KZG_VERIFY_MAX_PROOFS")]
    order = ["a required pointer NULL", "not a shape of", "proof_len not", "KZG_VERIFY_MAX_PROOFS", "n < 2", "pi_stride < n_public",
             "a shift or a public", "a key commitment off the curve", "a G2 input off the twist", "outside G1", "KZG_ERR_NO_SRS",
             "KZG_ERR_HIP"]
    doc_err = doc[doc.index("Errors, checked in this order"):]
    places = [doc_err.index(s) for s in order]
    assert places == sorted(places)
    for phrase in ("STRICTER THAN", "SIZE_MAX", "lookup proofs and next-row proofs", "proofs of different keys", "locating",
                   "hashing on the device", "2^-128"):
        assert phrase in doc, phrase


def test_the_restated_ladder_and_split_hold_the_constants_of_the_units_they_restate():
    """circuit_verify_kernels.hip restates verify_kernels.hip's GLV ladder and srs_update_kernels.hip's split: the same digits of
    beta as fk20_kernels.hip, verify_kernels.hip and the oracle, the same lambda as srs_update_kernels.hip and the oracle"""
    import verify_cells_oracle as VO
    csrc = os.path.join(ROOT, "kzg_poly_commit_exploration_amd", "csrc")
    read = lambda name: open(os.path.join(csrc, name)).read()  # noqa: E731
    digits = []
    for name in ("fk20_kernels.hip", "verify_kernels.hip", "circuit_verify_kernels.hip"):
        body = re.search(r"constexpr int32_t B\[13\] = \{([^}]*)\}", read(name)).group(1)
        digits.append([int(x.strip(), 16) if not x.strip().startswith("-") else -int(x.strip()[1:], 16) for x in body.split(",")])
    assert digits[0] == digits[1] == digits[2] == VO._BETA_DIGITS
    lam = []
    for name in ("srs_update_kernels.hip", "circuit_verify_kernels.hip"):
        m = re.search(r"kLambdaHi = (0x[0-9a-f]+)ULL, kLambdaLo = (0x[0-9a-f]+)ULL", read(name))
        lam.append(int(m.group(1), 16) << 64 | int(m.group(2), 16))
    assert lam[0] == lam[1] == VO.LAMBDA


def _tamper_eval(proof, t, log_ext):
    a, b = TR.layout(t, log_ext)["evals"]
    v = (int.from_bytes(proof[a:a + 32], "big") + 1) % R  # another canonical scalar
    return proof[:a] + v.to_bytes(32, "big") + proof[a + 32:]


def test_the_model_accepts_exactly_the_valid_batches(oracle):
    n, t, log_ext = 8, 3, 2
    (_, d0), (_, d1) = CP.case(oracle, n, t, log_ext, True, True), CP.case(oracle, n, t, log_ext, True, True, seed=1)
    c = d0["c"]
    assert d0["proof"] != d1["proof"] and d0["key48"] == d1["key48"]
    ms = [VB.member(d0), VB.member(d1)]
    for weights in ([1, 1], [3, R - 5], [0x1234567890ABCDEF << 64 | 77, 1]):
        assert VB.holds(VB.sums(c, log_ext, d0["key_s"], d0["key48"], ms, weights), CP.S)
    # each proof alone: the per-proof check
    for m in ms:
        assert VB.holds(VB.sums(c, log_ext, d0["key_s"], d0["key48"], [m], [1]), CP.S)
    # an evaluation changed, a commitment changed, a public input changed: rejected under weights that are not chosen for it
    bad_eval = VB.Member(_tamper_eval(d1["proof"], t, log_ext), d1["public"], d1["wire_s"], d1["z_s"], d1["t_s"], d1["w"])
    other = (d1["wire_s"][1] + 1) % R
    f = TR.split(d1["proof"], t, log_ext)
    wires = f["wires"][:48] + VB.TO.g1_scalar(oracle, other) + f["wires"][96:]
    bad_point = VB.Member(wires + d1["proof"][len(wires):], d1["public"], [d1["wire_s"][0], other] + d1["wire_s"][2:], d1["z_s"],
                          d1["t_s"], d1["w"])
    bad_pub = VB.Member(d1["proof"], [(d1["public"][0] + 1) % R] + d1["public"][1:], d1["wire_s"], d1["z_s"], d1["t_s"], d1["w"])
    for bad in (bad_eval, bad_point, bad_pub):
        for batch in ([bad], [ms[0], bad], [bad, ms[0]]):
            assert not VB.holds(VB.sums(c, log_ext, d0["key_s"], d0["key48"], batch, [7 + i for i in range(len(batch))]), CP.S)
    # W + D and W - D under weights (1, 1) cancel; under other weights they do not
    delta = 12345
    plus = VB.Member(d0["proof"], d0["public"], d0["wire_s"], d0["z_s"], d0["t_s"], d0["w"] + delta)
    minus = VB.Member(d0["proof"], d0["public"], d0["wire_s"], d0["z_s"], d0["t_s"], d0["w"] - delta)
    assert VB.holds(VB.sums(c, log_ext, d0["key_s"], d0["key48"], [plus, minus], [1, 1]), CP.S)
    assert not VB.holds(VB.sums(c, log_ext, d0["key_s"], d0["key48"], [plus, minus], [1, 2]), CP.S)


def test_the_models_public_input_rule_is_linearise_oracles():
    n, public = 8, [5, 0, R - 1, 77, 1 << 200]
    w = VB.NO.domain_root(3)
    for zeta in (2, R - 3, 0x1234567 << 100, 1, w, pow(w, 4, R), pow(w, 6, R)):
        assert VB.public_input_at(n, public, zeta) == VB.LN.public_input_at(n, public, zeta), zeta
    assert VB.public_input_at(n, [], 9) == 0


def test_the_model_accepts_a_custom_circuits_proof(oracle):
    n, t, log_ext, exps = CC.SHAPES[1]
    case = CC.case(n, t, log_ext, exps)
    d = CC.memo(("proof", n, t, log_ext, exps), lambda: CX.prove(oracle, case.cc, log_ext, case.zero, CP.S))
    c = case.cc.circuit
    m = VB.member(d)
    assert VB.holds(VB.sums(c, log_ext, d["key_s"], d["key48"], [m, m], [5, 9], cc=case.cc), CP.S)
    plain = 2 * t + 2  # ... and not under the plain statement of the key's first 2 t + 2 commitments
    assert not VB.holds(VB.sums(c, log_ext, d["key_s"][:plain], d["key48"][:plain], [m], [1]), CP.S)
