"""GPU: kzg_circuit_verify_proofs_batch / _lincomb against the host verifier and against the trapdoor
model of tests/circuit_verify_batch_oracle.py.

Proofs come from tests/transcript_oracle.py (circuit_proof_cases' cache) and tests/circuit_custom_oracle.py, so every point of a
proof is [c]G with a known scalar and the three sums of the hook are [p0]G, [p1]G, [p2]G for scalars the model computes.
Shapes (n, t, log_ext): (2, 3, 2); (8, 3, 2) with and without public inputs; (256, 3, 2) blinded with public inputs; (64, 7, 3),
t + e = 15 products per proof; (4096, 2, 2); the custom S-box circuit (8, 3, 3) with g = 2.  Counts 1, 2, 17 (one past the 16
terms a lane sums per level) and 65 (one past a workgroup), built by repeating the distinct proofs of a shape; at (8, 3, 2) four
distinct proofs with three distinct sets of public inputs (the witness shifted by a constant keeps the key).  Two proofs with
different public inputs, plain and under the custom statement at (8, 3, 2) with g = 2, are held to the single verifier one by one.

zeta inside the domain H: the challenges are hashed, so no proof reaches it; the test entry
kzg_circuit_verify_proofs_lincomb_challenges takes caller challenges, and the three points are held to the model under the same
challenges at zeta = 1, zeta = w^i with i below and past n_public, and off H."""
import ctypes as C

import numpy as np
import pytest

import bigint_twin as T
import blind_oracle as BO
import circuit_custom_cases as CC
import circuit_custom_oracle as CX
import circuit_oracle as CO
import circuit_proof_cases as CP
import circuit_verify_batch_oracle as VB
import kzg_poly_commit_exploration_amd as K
import transcript_oracle as TR
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu
R = VB.R
SRS = 4096 + 16  # the engine tests/test_circuit_proof_gpu.py uses
COUNTS = (1, 2, 17, 65)
PLAIN = [(2, 3, 2, True, False), (8, 3, 2, True, True), (8, 3, 2, False, True), (256, 3, 2, True, True), (64, 7, 3, True, True),
         (4096, 2, 2, True, True)]
SHAPES = PLAIN + ["custom"]
CUSTOM_SMALL = (8, 3, 2, ((1, 1, 1), (3, 0, 0)))  # "custom_small": the custom statement at the plain (8, 3, 2), d_max = e - 1
_CACHE = {}


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _setup(oracle):
    return _memo("setup", lambda: (np.stack([oracle.p1_generator()]), np.stack([K.srs_g2_at(T.BENCH_SECRET_BE, j) for j in range(3)])))


def _shifted(c, by):
    """c's key with another witness and other public inputs: every wire value plus `by` keeps the copy constraints"""
    wires = [[(x + by) % R for x in col] for col in c.wires]
    v = CO.Circuit(c.ks, wires, c.sigmas, c.q_lin, c.q_mul, c.q_const, [0] * c.n)
    v.pi = [(-x) % R for x in CO.gate_rows(v)]
    assert CO.gate_rows(v) == [0] * c.n
    return v


def _shifted_custom(cc, by):
    """_shifted for a custom circuit: the public inputs take up the custom terms' change too"""
    c = cc.circuit
    wires = [[(x + by) % R for x in col] for col in c.wires]
    v = CX.CustomCircuit(CO.Circuit(c.ks, wires, c.sigmas, c.q_lin, c.q_mul, c.q_const, [0] * c.n), cc.q_custom, cc.exps)
    v.circuit.pi = [(-x) % R for x in CX.gate_rows(v)]
    assert CX.gate_rows(v) == [0] * c.n
    return v


class Shape:
    """the statement and the distinct valid proofs of one shape, with what the model needs"""

    def __init__(self, oracle, which):
        self.cc = None
        if which in ("custom", "custom_small"):
            n, t, log_ext, exps = CC.SBOX if which == "custom" else CUSTOM_SMALL
            case = CC.case(n, t, log_ext, exps)
            if which == "custom":
                ds = [CX.prove(oracle, case.cc, log_ext, bl, CP.S) for bl in (case.zero, case.blinders(3))]
            else:  # two witnesses of one key with different public inputs
                ds = [CX.prove(oracle, cc, log_ext, case.zero, CP.S) for cc in (case.cc, _shifted_custom(case.cc, 1))]
                assert ds[0]["public"] != ds[1]["public"]
            self.cc, self.c = case.cc, case.cc.circuit
            self.exps = np.array(exps, dtype=np.uint8)
        else:
            n, t, log_ext, with_pi, blinded = which
            ds = [CP.case(oracle, n, t, log_ext, with_pi, blinded)[1]]
            if blinded:
                ds.append(CP.case(oracle, n, t, log_ext, with_pi, blinded, seed=1)[1])
            self.c, self.exps = ds[0]["c"], None
            if with_pi and n == 8:
                for by in (1, 2):
                    ds.append(TR.prove(oracle, _shifted(self.c, by), log_ext, BO.Blinders.random(t, log_ext, 50 + by), CP.S))
                assert len({tuple(d["public"]) for d in ds}) == 3
        self.n, self.t, self.log_ext = n, t, log_ext
        self.key_s, self.key48 = ds[0]["key_s"], ds[0]["key48"]
        assert all(d["key48"] == self.key48 for d in ds)
        self.key = [K.G1Point.uncompress(k) for k in self.key48]
        self.shifts = [K.Scalar(k) for k in self.c.ks]
        self.members = [VB.member(d) for d in ds]
        assert len({m.proof for m in self.members}) == len(self.members)
        self._single, self._contrib, self._rows = {}, {}, {}  # (the last two keep their member alive: ids are not reused)

    def batch(self, count):
        return [self.members[k % len(self.members)] for k in range(count)]

    def args(self, members):
        """the first arguments of the Python calls; the public inputs as (count, n_public, 4) rows, a member's made once"""
        pub = None
        if members and members[0].public:
            for m in members:
                if id(m) not in self._rows:
                    self._rows[id(m)] = (m, K._scalar_rows([K.Scalar(p) for p in m.public]))
            pub = np.stack([self._rows[id(m)][1] for m in members])
        return self.key, self.n, self.log_ext, self.shifts, pub, [m.proof for m in members]

    def single(self, oracle, m):
        """the host verifier's answer, once per distinct (proof, public inputs)"""
        key = (m.proof, tuple(m.public))
        if key not in self._single:
            g1, g2 = _setup(oracle)
            pub = [K.Scalar(p) for p in m.public]
            if self.cc is None:
                ok = K.circuit_verify_proof(self.key, self.n, self.log_ext, self.shifts, pub, m.proof, g1, g2)
            else:
                ok = K.circuit_custom_verify_proof(self.key, self.n, self.log_ext, self.exps, self.shifts, pub, m.proof, g1, g2)
            self._single[key] = ok
        return self._single[key]

    def model(self, oracle, members, weights):
        """the model's three points; a member's weight-free part is computed once"""
        for m in members:
            if id(m) not in self._contrib:
                self._contrib[id(m)] = (m, VB.contribution(self.c, self.log_ext, self.key_s, self.key48, m, self.cc))
        return VB.points(oracle, VB.combine(self.n, [self._contrib[id(m)][1] for m in members], weights))


def _shape(oracle, which):
    return _memo(("shape", which if isinstance(which, str) else tuple(which)), lambda: Shape(oracle, which))


def _batch(e, oracle, sh, members, **kw):
    return e.circuit_verify_proofs_batch(*sh.args(members), _setup(oracle)[1], exponents=sh.exps, **kw)


def _hook(e, oracle, sh, members, weights, **kw):
    return e.circuit_verify_proofs_lincomb(*sh.args(members), _setup(oracle)[1], [K.Scalar(x) for x in weights], exponents=sh.exps, **kw)


def _weights(count, seed):
    rnd = np.random.default_rng(seed)
    full = lambda: int.from_bytes(rnd.bytes(32), "big") % R  # noqa: E731
    special = [1, R - 1, 0, 2]
    return [special[k] if k < len(special) and count > 4 else full() for k in range(count)]


def _with_eval(m, sh, i=0):
    """evaluation i replaced by another canonical scalar"""
    a, _ = TR.layout(sh.t, sh.log_ext)["evals"]
    v = (int.from_bytes(m.proof[a + 32 * i:a + 32 * i + 32], "big") + 1) % R
    return VB.Member(m.proof[:a + 32 * i] + v.to_bytes(32, "big") + m.proof[a + 32 * i + 32:], m.public, m.wire_s, m.z_s, m.t_s, m.w)


def _with_wire(oracle, m, j=1):
    """wire commitment j replaced by another G1 point"""
    other = (m.wire_s[j] + 1) % R
    proof = m.proof[:48 * j] + TO.g1_scalar(oracle, other) + m.proof[48 * j + 48:]
    return VB.Member(proof, m.public, m.wire_s[:j] + [other] + m.wire_s[j + 1:], m.z_s, m.t_s, m.w)


def _with_w(oracle, m, delta):
    return VB.Member(m.proof[:-48] + TO.g1_scalar(oracle, m.w + delta), m.public, m.wire_s, m.z_s, m.t_s, m.w + delta)


@pytest.mark.parametrize("which", SHAPES, ids=str)
def test_the_hooks_three_points_are_the_models_and_valid_batches_are_accepted(engines, oracle, which):
    e, sh = engines.bench_srs(SRS), _shape(oracle, which)
    for count in COUNTS:
        ms = sh.batch(count)
        assert all(sh.single(oracle, m) for m in ms)
        weights = _weights(count, 100 + count)
        ok, bad, pts = _hook(e, oracle, sh, ms, weights)
        assert ok and bad is None, count
        assert [p.compress() for p in pts] == sh.model(oracle, ms, weights), count
        assert _batch(e, oracle, sh, ms) == (True, None), count


@pytest.mark.parametrize("which", SHAPES, ids=str)
def test_one_changed_proof_rejects_the_batch_as_the_host_verifier_rejects_the_proof(engines, oracle, which):
    e, sh = engines.bench_srs(SRS), _shape(oracle, which)
    m0 = sh.members[0]
    for change in (_with_eval(m0, sh), _with_eval(m0, sh, 2 * sh.t - 1), _with_wire(oracle, m0)):
        assert not sh.single(oracle, change)
        for count in COUNTS:
            for at in sorted({0, count // 2, count - 1}):
                ms = sh.batch(count)
                ms[at] = change
                want = all(sh.single(oracle, m) for m in ms)
                assert not want
                assert _batch(e, oracle, sh, ms) == (False, None), (count, at)  # only the pairing fails: no index
            if count == 17:  # the hook computes the model's points for an invalid batch too
                weights = _weights(count, 7)
                ok, bad, pts = _hook(e, oracle, sh, ms, weights)
                assert not ok and bad is None and [p.compress() for p in pts] == sh.model(oracle, ms, weights)


@pytest.mark.parametrize("which", [PLAIN[1], "custom_small"], ids=str)
def test_two_proofs_with_different_public_inputs_as_one_by_one(engines, oracle, which):
    """(8, 3, 2), plain and custom: the batch hashes the statement's bytes in front of the public inputs once and finishes a copy of
    that state per proof, the single verifier hashes both halves per call.  A batch of two proofs with different public inputs is
    accepted exactly when both are accepted one by one -- in either order, and with one proof's or both proofs' public inputs
    replaced by the other's"""
    e, sh = engines.bench_srs(SRS), _shape(oracle, which)
    a = sh.members[0]
    b = next(m for m in sh.members if m.public != a.public)
    under = lambda m, other: VB.Member(m.proof, other.public, m.wire_s, m.z_s, m.t_s, m.w)  # noqa: E731
    a_wrong, b_wrong = under(a, b), under(b, a)
    assert sh.single(oracle, a) and sh.single(oracle, b) and not sh.single(oracle, a_wrong) and not sh.single(oracle, b_wrong)
    for ms in ([a, b], [b, a], [a, b_wrong], [a_wrong, b], [a_wrong, b_wrong], [b_wrong, a]):
        want = all(sh.single(oracle, m) for m in ms)
        assert _batch(e, oracle, sh, ms) == (want, None), [m is a or m is b for m in ms]


@pytest.mark.parametrize("which", [PLAIN[1], PLAIN[2], "custom"], ids=str)
def test_zeta_on_the_domain_through_the_challenges_entry(engines, oracle, which):
    """the scalar kernels' special paths: L_0(1) = 1, L_0(w^i) = 0, PI(w^i) = PI_i inside the public rows and 0 past them -- one
    batch of 65 proofs (two workgroups of k_cvb_lin) in which zeta differs from proof to proof, so that the shared inversions mix
    substituted and real denominators"""
    e, sh = engines.bench_srs(SRS), _shape(oracle, which)
    w = VB.NO.domain_root(VB.NO.log2_exact(sh.n))
    rnd = np.random.default_rng(77)
    full = lambda: int.from_bytes(rnd.bytes(32), "big") % R  # noqa: E731
    zetas = [1, w, pow(w, sh.n - 1, R), full(), pow(w, 3, R), 1, full(), pow(w, 5, R)]
    ms = sh.batch(65)
    hashed = {}
    challenges = []
    for k, m in enumerate(ms):
        if id(m) not in hashed:
            hashed[id(m)] = (TR.challenges(sh.n, sh.t, sh.log_ext, sh.c.ks, sh.key48, m.public, m.proof) if sh.cc is None else
                             CX.challenges(sh.n, sh.t, sh.log_ext, sh.cc.exps, sh.c.ks, sh.key48, m.public, m.proof))
        beta, gamma, alpha, zeta, v = hashed[id(m)]
        if k % 9 != 8:  # every ninth proof keeps its own transcript: a valid proof among the others
            zeta = zetas[k % len(zetas)]
        challenges.append((beta, gamma, alpha, zeta, v))
    weights = _weights(65, 21)
    ok, bad, pts = _hook(e, oracle, sh, ms, weights, challenges=[[K.Scalar(c) for c in five] for five in challenges])
    assert bad is None and not ok  # (the evaluations were made for another zeta)
    contribs = [VB.contribution(sh.c, sh.log_ext, sh.key_s, sh.key48, m, sh.cc, challenges=five) for m, five in zip(ms, challenges)]
    assert [p.compress() for p in pts] == VB.points(oracle, VB.combine(sh.n, contribs, weights))
    # with every proof's own challenges the entry is the hashed one
    own = [[K.Scalar(c) for c in hashed[id(m)]] for m in ms]
    ok, bad, pts = _hook(e, oracle, sh, ms, weights, challenges=own)
    assert ok and [p.compress() for p in pts] == sh.model(oracle, ms, weights)


def test_the_weights_matter(engines, oracle):
    e, sh = engines.bench_srs(SRS), _shape(oracle, PLAIN[1])
    m = sh.members[0]
    pair = [_with_w(oracle, m, 12345), _with_w(oracle, m, -12345)]
    assert not sh.single(oracle, pair[0]) and not sh.single(oracle, pair[1])
    ok, bad, pts = _hook(e, oracle, sh, pair, [1, 1])
    assert ok and bad is None and [p.compress() for p in pts] == sh.model(oracle, pair, [1, 1])  # W + D and W - D cancel
    assert not _hook(e, oracle, sh, pair, [1, 2])[0]
    for _ in range(4):  # fresh weights on every call
        assert _batch(e, oracle, sh, pair) == (False, None)


def test_undecodable_proofs_and_points_outside_g1_are_invalid_not_errors(engines, oracle):
    e, sh = engines.bench_srs(SRS), _shape(oracle, PLAIN[1])
    L = TR.layout(sh.t, sh.log_ext)
    m = sh.members[0]

    def put(at, data, base=m):
        return VB.Member(base.proof[:at] + data + base.proof[at + len(data):], base.public, base.wire_s, base.z_s, base.t_s, base.w)

    big_eval = put(L["evals"][0] + 32, R.to_bytes(32, "big"))  # r itself: the least value that is not canonical
    no_point = put(L["chunks"][0], bytes(48))  # the compression bit is not set
    x_big = put(L["w"][0], bytes([0x9F]) + b"\xff" * 47)  # x >= p
    changes = [big_eval, no_point, x_big]
    for q, tp in TO.torsion_points().items():  # on the curve, outside G1: a commitment shifted by a torsion point
        for name, scalar in (("z", m.z_s), ("w", m.w), ("wires", m.wire_s[0])):
            changes.append(put(L[name][0], T.g1_compress(T.g1_add(T.g1_mul(T.G1, scalar % R), tp))))
    g1, g2 = _setup(oracle)
    for i, change in enumerate(changes):
        for count, ats in ((1, [0]), (17, [16]), (65, [40, 64]), (65, [0, 3]))[:4 if i < 3 else 2]:
            ms = sh.batch(count)
            for at in ats:
                ms[at] = change
            assert _batch(e, oracle, sh, ms) == (False, ats[0]), (count, ats)
            ok, bad, pts = _hook(e, oracle, sh, ms, _weights(count, 3))
            assert not ok and bad == ats[0] and all(p.compress() == TR.INFINITY48 for p in pts)
    # the least proof over the kinds: an evaluation at 9, a torsion point at 5, an undecodable point at 30
    ms = sh.batch(65)
    ms[9], ms[5], ms[30] = big_eval, changes[-1], no_point
    assert _batch(e, oracle, sh, ms) == (False, 5)
    ms[5] = sh.members[1]
    assert _batch(e, oracle, sh, ms) == (False, 9)
    # the host verifier makes no subgroup check: the point at infinity as a commitment decodes and is in G1 for both
    inf = put(L["wires"][0], TR.INFINITY48)
    assert _batch(e, oracle, sh, [m, inf]) == (False, None) and not sh.single(oracle, inf)
    assert _batch(e, oracle, sh, []) == (True, None)
    ok, bad, pts = _hook(e, oracle, sh, [], [])
    assert ok and bad is None and all(p.compress() == TR.INFINITY48 for p in pts)


def _raw(e, sh, members, g2, n_public=None, pub=None):
    """the C call's arguments as a list the caller edits, and what has to stay alive"""
    if pub is None:
        pub = np.stack([K._scalar_rows([K.Scalar(p) for p in m.public]) for m in members])
    keep, count, a = e._circuit_verify_batch_args(sh.key, sh.n, sh.log_ext, sh.shifts, pub, [m.proof for m in members], g2, sh.exps,
                                                  n_public)
    return keep, list(a)


# positions in the argument list behind ctx
KEY, N, T_, LOG_EXT, G, EXPS, SHIFTS, PUB, N_PUBLIC, STRIDE, PROOFS, PROOF_LEN, COUNT, G2, G2_STRIDE = range(15)


def test_statuses_in_the_documented_order_leave_valid_untouched(engines, oracle):
    e, sh = engines.bench_srs(SRS), _shape(oracle, PLAIN[1])
    lib = K.load_library()
    g2 = _setup(oracle)[1]
    ms = sh.batch(3)
    keep, base = _raw(e, sh, ms, g2)
    big = np.array([0xFFFFFFFFFFFFFFFF] * 4, dtype=np.uint64)
    ks_bad = keep[2].copy()
    ks_bad[1] = big
    pub_bad = keep[3].copy()
    pub_bad[1, 2] = big
    key_bad = keep[0].copy()
    key_bad[2, 6] ^= np.uint64(1)
    g2_bad = g2.copy()
    g2_bad[1, 0] ^= np.uint64(1)
    # (what to change, what kzg_last_error then says), in the order the header documents
    steps = [({SHIFTS: None}, b"pointer is NULL"),
             ({T_: 1}, b"not a shape"),
             ({PROOF_LEN: base[PROOF_LEN] + 1}, b"proof_len"),
             ({COUNT: K.KZG_VERIFY_MAX_PROOFS + 1}, b"KZG_VERIFY_MAX_PROOFS"),
             ({N: 1, N_PUBLIC: 1}, b"n < 2"),
             ({STRIDE: base[N_PUBLIC] - 1}, b"pi_stride"),
             ({SHIFTS: K._ptr(ks_bad)}, b"a shift is not below r"),
             ({PUB: K._ptr(pub_bad)}, b"proof 1: public input 2"),
             ({KEY: K._ptr(key_bad)}, b"key commitment 2 is not on the curve"),
             ({G2: K._ptr(g2_bad)}, b"setup_g2[1] is not on the twist")]

    def call(changes, hook_weights=None):
        a = list(base)
        for at, v in changes.items():
            a[at] = v
        ok, bad = C.c_int(7), C.c_size_t(5)
        if hook_weights is None:
            rc = lib.kzg_circuit_verify_proofs_batch(e._h, *a, C.byref(ok), C.byref(bad))
        else:
            out = np.zeros((3, 18), dtype=np.uint64)
            rc = lib.kzg_circuit_verify_proofs_lincomb(e._h, *a, K._ptr(hook_weights), K._ptr(out), C.byref(ok), C.byref(bad))
        return rc, ok.value, lib.kzg_last_error(e._h)

    assert call({})[:2] == (K.KZG_OK, 1)
    for i, (changes, says) in enumerate(steps):
        both = {**steps[i + 1][0], **changes} if i + 1 < len(steps) and not (set(changes) & set(steps[i + 1][0])) else changes
        for ch in (changes, both):  # alone, and together with the next one: the earlier check answers
            rc, ok, msg = call(ch)
            assert rc == K.KZG_ERR_INVALID_ARG and ok == 7 and says in msg, (i, msg)
    w = np.stack([K.Scalar(1).limbs(), big, K.Scalar(2).limbs()])
    rc, ok, msg = call({}, w)
    assert rc == K.KZG_ERR_INVALID_ARG and ok == 7 and b"weight 1 is not below r" in msg
    rc, ok, msg = call({G2: K._ptr(g2_bad)}, w)
    assert rc == K.KZG_ERR_INVALID_ARG and b"twist" in msg  # the weights are looked at last
    # a key commitment outside G1: found by the device
    for q, tp in list(TO.torsion_points().items())[:2]:
        key_out = keep[0].copy()
        key_out[4] = np.array(T.g1_to_blst_p1_limbs(T.g1_add(T.g1_mul(T.G1, sh.key_s[4]), tp)), dtype=np.uint64)
        rc, ok, msg = call({KEY: K._ptr(key_out)})
        assert rc == K.KZG_ERR_INVALID_ARG and ok == 7 and b"key commitment 4 is not in G1" in msg, q
    # after the errors the context still serves a good batch
    assert call({})[:2] == (K.KZG_OK, 1) and _batch(e, oracle, sh, sh.batch(17)) == (True, None)
    nosrs = K.Engine(0)
    try:
        with pytest.raises(K.KzgError) as ei:
            _batch(nosrs, oracle, sh, ms)
        assert ei.value.status == K.KZG_ERR_NO_SRS
    finally:
        nosrs.close()


def test_public_inputs_at_a_stride_of_their_own(engines, oracle):
    e, sh = engines.bench_srs(SRS), _shape(oracle, PLAIN[1])
    ms = sh.batch(17)
    n_public = len(ms[0].public)
    pub = np.full((17, n_public + 3, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)  # what lies between the proofs' inputs is not read
    for k, m in enumerate(ms):
        pub[k, :n_public] = K._scalar_rows([K.Scalar(p) for p in m.public])
    g2 = _setup(oracle)[1]
    assert e.circuit_verify_proofs_batch(sh.key, sh.n, sh.log_ext, sh.shifts, pub, [m.proof for m in ms], g2, n_public=n_public) == (True, None)
    weights = _weights(17, 5)
    ok, bad, pts = e.circuit_verify_proofs_lincomb(sh.key, sh.n, sh.log_ext, sh.shifts, pub, [m.proof for m in ms], g2,
                                                   [K.Scalar(x) for x in weights], n_public=n_public)
    assert ok and [p.compress() for p in pts] == sh.model(oracle, ms, weights)
    pub[4, 1] = K.Scalar(ms[4].public[1] + 1).limbs()
    assert e.circuit_verify_proofs_batch(sh.key, sh.n, sh.log_ext, sh.shifts, pub, [m.proof for m in ms], g2, n_public=n_public) == (False, None)


def test_workspaces_regrown_and_reused_on_a_fresh_context(oracle):
    sh = _shape(oracle, PLAIN[1])
    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(16)
    try:
        for count in (2, 65, 3, 17, 1):  # a larger call regrows them, a smaller one after it reads the same buffers
            ms = sh.batch(count)
            weights = _weights(count, 40 + count)
            ok, bad, pts = _hook(e, oracle, sh, ms, weights)
            assert ok and [p.compress() for p in pts] == sh.model(oracle, ms, weights), count
            ms[count - 1] = _with_eval(ms[count - 1], sh)
            assert _batch(e, oracle, sh, ms) == (False, None), count
    finally:
        e.close()


def test_two_device_contexts(oracle):
    sh = _shape(oracle, PLAIN[1])
    ms = sh.batch(17)
    rep = K.Engine(devices=[0, 0], replicate=True)
    try:
        rep.srs_generate(T.BENCH_SECRET_BE, 128)
        weights = _weights(17, 9)
        ok, bad, pts = _hook(rep, oracle, sh, ms, weights)
        assert ok and [p.compress() for p in pts] == sh.model(oracle, ms, weights)
        ms[8] = _with_wire(oracle, ms[8])
        assert _batch(rep, oracle, sh, ms) == (False, None)
    finally:
        rep.close()
    split = K.Engine(devices=[0, 0])
    try:
        split.srs_generate(T.BENCH_SECRET_BE, 128)
        with pytest.raises(K.KzgError) as ei:
            _batch(split, oracle, sh, sh.batch(2))
        assert ei.value.status == K.KZG_ERR_INVALID_ARG and b"range-split" in K.load_library().kzg_last_error(split._h)
    finally:
        split.close()
