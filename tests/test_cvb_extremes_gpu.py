"""GPU: the batch verifier's Fr kernels and GLV ladders (csrc/circuit_verify_kernels.hip) at their edges, through
kzg_circuit_verify_proofs_lincomb_challenges: the three points under caller weights and caller challenges against
tests/circuit_verify_batch_oracle.py, bit for bit.  The statements are synthetic (tests/cvb_extremes.py: key commitments and proof
points [c]G with c known, free evaluations and public inputs); no proof here is valid, and none needs to be.

  * magnitudes: challenges, evaluations, weights and public inputs from the half values, the digit-extremal images and the extremal
    multipliers with another phase per proof; the compensated families (every term of the chained sums of one sign); 65 rows of r - 1
    under k_vc_fr_sum;
  * the split and the ladder: every split target as a weight (cvb_emit_glv), as the sum of two weights through a wrap mod r
    (k_cvb_key_split) and as each of the stage-2 scalars (k_cvb_stage2);
  * points at infinity in stage 2; zero challenges; k_cvb_public's rounds with zeta on the domain.
Batches of 1 localise a failure; 65 crosses a workgroup of k_cvb_lin, the lane arithmetic of k_cvb_scalars and k_vc_fr_sum's levels.
Shapes (n, t, log_ext): (2, 3, 2), (8, 3, 2), (64, 7, 3), (256, 3, 2) and the custom (8, 4, 3) with g = 8 and exponent rows of degree 7."""
import numpy as np
import pytest

import bigint_twin as T
import circuit_verify_batch_oracle as VB
import cvb_extremes as CE
import fr_extremes as FE
import kzg_poly_commit_exploration_amd as K

pytestmark = pytest.mark.gpu
R = VB.R
SRS = 4096 + 16
_CACHE = {}


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _g2():
    return _memo("g2", lambda: np.stack([K.srs_g2_at(T.BENCH_SECRET_BE, j) for j in range(3)]))


def _args(oracle, which):
    """the statement and its arguments of the Python call, once per shape"""
    def make():
        st = CE.statement(oracle, which)
        return (st, [K.G1Point.uncompress(k) for k in st.key48], [K.Scalar(k) for k in st.ks],
                None if st.exps is None else np.array(st.exps, dtype=np.uint8))

    return _memo(("args", which), make)


def _run(e, oracle, which, records, scalars=None, stride=None):
    """records: (five, rho, evals, public) per proof, plain integers; scalars: the proof points' scalars per proof (the statement's
    stock in turn when not given); stride: the public inputs as a (count, stride, 4) array.  The hook's points against the model's"""
    st, key, shifts, exps = _args(oracle, which)
    members = [st.member(evals, public, st.stock[k % 3] if scalars is None else scalars[k])
               for k, (_, _, evals, public) in enumerate(records)]
    fives, weights = [five for five, _, _, _ in records], [rho for _, rho, _, _ in records]
    n_public = len(records[0][3])
    kw = {}
    if stride is not None:
        pub = np.zeros((len(records), stride, 4), dtype=np.uint64)
        for k, m in enumerate(members):
            if n_public:
                pub[k, :n_public] = K._scalar_rows([K.Scalar(p) for p in m.public])
        kw["n_public"] = n_public
    else:
        pub = [[K.Scalar(p) for p in m.public] for m in members] if n_public else None
    ok, bad, pts = e.circuit_verify_proofs_lincomb(key, st.n, st.log_ext, shifts, pub, [m.proof for m in members], _g2(),
                                                   [K.Scalar(x) for x in weights], exponents=exps,
                                                   challenges=[[K.Scalar(c) for c in five] for five in fives], **kw)
    assert bad is None
    want = VB.points(oracle, VB.combine(st.n, [st.contribution(m, five) for m, five in zip(members, fives)], weights))
    assert [p.compress() for p in pts] == want
    return ok


def _cycled(which, oracle, count, n_public, values=None, first=0):
    st = CE.statement(oracle, which)
    values = CE.pool() if values is None else values
    out = []
    for k in range(first, first + count):
        five, evals, rho, public = CE.cycled(values, st.t, k, n_public)
        out.append((five, rho, evals, public))
    return out


@pytest.mark.parametrize("which", list(CE.SHAPES))
def test_magnitudes_cycled_through_the_extremal_families(engines, oracle, which):
    e, st = engines.bench_srs(SRS), CE.statement(oracle, which)
    n_public = min(st.n, 5)
    for k in range(4):  # one proof at a time: a failure names the phase
        _run(e, oracle, which, _cycled(which, oracle, 1, n_public, first=9 * k))
    _run(e, oracle, which, _cycled(which, oracle, 65, n_public))
    _run(e, oracle, which, _cycled(which, oracle, 17, 0, first=3))


@pytest.mark.parametrize("h", [CE.HP, CE.HM], ids=["plus", "minus"])
@pytest.mark.parametrize("which", list(CE.SHAPES))
def test_magnitudes_compensated_every_term_of_one_sign(engines, oracle, which, h):
    """the three-term sums of k_cvb_lin, the g0 chain of k_cvb_scalars with two of its constant's terms, and the lanes' total of
    k_cvb_public (64 public inputs at n = 256, n below that), every term congruent to +-r/2 with the one sign"""
    e, st = engines.bench_srs(SRS), CE.statement(oracle, which)
    n_public = min(st.n, 64)
    wi = [pow(st.w, i, R) for i in range(n_public)]
    values = CE.pool()
    records = []
    for k in range(17):
        kind = "lin" if k % 2 == 0 else "g0"
        five, evals = CE.compensated(kind, st.ks, k, h)
        if kind == "lin":
            public = CE.compensated_public(five[3], wi, h)
        else:
            public = CE.public_for(-FE.multiplier_for(h) % R, st.n, five[3], n_public)
        records.append((five, CE.cycle(values, k, 0), evals, public))
    _run(e, oracle, which, records[:1])
    _run(e, oracle, which, records[1:2])
    _run(e, oracle, which, records)


def test_sixty_five_rows_of_r_minus_one_under_the_key_sides_sum(engines, oracle):
    e = engines.bench_srs(SRS)
    records = [(five, 1, [R - 1] + evals[1:], public) for five, _, evals, public in _cycled("n8", oracle, 65, 5)]
    _run(e, oracle, "n8", records)


def _v_one(which, oracle, k):
    five, rho, evals, public = _cycled(which, oracle, 1, 3, first=k)[0]
    return five[:4] + (1,), evals, public


@pytest.mark.parametrize("part", [0, 1])
def test_split_targets_as_weights_and_as_sums_of_weights(engines, oracle, part):
    """v = 1: the scalars of the wires and of E are rho itself (cvb_emit_glv, and the host's split for F), and q_C's row of P1 is the
    sum of the weights: rho_0 + rho_1 = target through a wrap mod r reaches k_cvb_key_split"""
    e = engines.bench_srs(SRS)
    for i, target in enumerate(CE.SPLIT_TARGETS[part::2]):
        five, evals, public = _v_one("n8", oracle, i)
        _run(e, oracle, "n8", [(five, target, evals, public)])
        five1, evals1, public1 = _v_one("n8", oracle, i + 40)
        _run(e, oracle, "n8", [(five, R - 1, evals, public), (five1, (target + 1) % R, evals1, public1)])


@pytest.mark.parametrize("which", ["n8", "n2"])
def test_split_targets_as_stage_two_scalars(engines, oracle, which):
    """zeta = -target (E's scalar), -target / w (D's) and target / (1 + w) (F's in P1); at n = 2, 1 + w = 0 and that scalar is zero for
    every zeta"""
    e, st = engines.bench_srs(SRS), CE.statement(oracle, which)
    zetas = []
    for target in CE.SPLIT_TARGETS:
        zetas += [-target % R, -target * pow(st.w, -1, R) % R]
        if which != "n2":
            zetas.append(target * pow(1 + st.w, -1, R) % R)
    records = []
    for k, zeta in enumerate(zetas):
        five, rho, evals, public = _cycled(which, oracle, 1, 2, first=k)[0]
        records.append((five[:3] + (zeta,) + five[4:], rho or 5, evals, public))
    for rec in records:
        _run(e, oracle, which, [rec])
    _run(e, oracle, which, records)


@pytest.mark.parametrize("count", [1, 17])
def test_points_at_infinity_in_stage_two(engines, oracle, count):
    """W at infinity makes F_k infinite, [z] at infinity E_k, rho = 0 all of D_k, E_k, F_k"""
    e, st = engines.bench_srs(SRS), CE.statement(oracle, "n8")
    t, base = st.t, st.stock[0]
    no_w, no_z = base[:-1] + [0], base[:t] + [0] + base[t + 1:]
    points = {"w": no_w, "z": no_z, "both": no_z[:-1] + [0], "rho": base}
    for case in points:
        records, scalars = [], []
        for k, rec in enumerate(_cycled("n8", oracle, count, 3, first=2)):
            special = k in (0, 8, 16)
            five, rho, evals, public = rec
            records.append((five, 0 if special and case == "rho" else (rho or 7), evals, public))
            scalars.append(points[case] if special else st.stock[k % 3])
        _run(e, oracle, "n8", records, scalars)


@pytest.mark.parametrize("which", ["n8", "custom"])
def test_zero_challenges(engines, oracle, which):
    """beta, gamma, alpha, zeta, v = 0 are below r: each in turn, then all five.  v = 0: every power of v is zero; zeta = 0: every
    stage-2 scalar is zero and L_0(0) = 1 / n"""
    e = engines.bench_srs(SRS)
    records = []
    for k, zero in enumerate([(0,), (1,), (2,), (3,), (4,), (0, 1, 2, 3, 4)]):
        five, rho, evals, public = _cycled(which, oracle, 1, 5, CE.plain_pool(3)[3:], first=k)[0]
        records.append((tuple(0 if i in zero else c for i, c in enumerate(five)), rho, evals, public))
    for rec in records:
        _run(e, oracle, which, [rec])
    _run(e, oracle, which, records + _cycled(which, oracle, 11, 5))


@pytest.mark.parametrize("n_public", [0, 1, 63, 64, 65, 127, 128, 129, 255, 256])
def test_public_input_rounds_with_zeta_on_the_domain(engines, oracle, n_public):
    """k_cvb_public at n = 256 (four rounds): zeta = w^i hit in round 0, in a middle round, in the last, partly dead round and just
    past the public rows (no hit there: PI is the ordinary sum and L_0 = 0), zeta differing from proof to proof in a batch of 65, the
    public inputs from the extremal pool so that acc holds +-r/2 terms when the hit lane drops out"""
    e, st = engines.bench_srs(SRS), CE.statement(oracle, "n256")
    where = [0, 63, 64, 255] + ([n_public - 1] if n_public else []) + ([n_public] if n_public < st.n else [])
    zetas = [pow(st.w, i, R) for i in where] + [0x1234567890ABCDEF1234567890ABCDEF % R]
    records = []
    for k, (five, rho, evals, public) in enumerate(_cycled("n256", oracle, 65, n_public)):
        records.append((five[:3] + (zetas[k % len(zetas)],) + five[4:], rho, evals, public))
    _run(e, oracle, "n256", records, stride=256)
    if n_public in (65, 129):
        for k in range(len(zetas)):
            _run(e, oracle, "n256", records[k:k + 1], stride=256)
