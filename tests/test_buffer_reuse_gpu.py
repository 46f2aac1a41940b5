"""GPU: one engine driven through every family of device and pinned buffers in the order small, large, small, so that each
buffer is created, grown, and then reused while larger than the call needs ("Who owns which memory"),
with the SRS replaced in the middle: the nine MSM-side families at an SRS of 256 points, then -- after the SRS has grown to 2048
points -- the prover families (grand products, lookups, transforms, evaluation-form and Lagrange-basis calls, the coset extension
and the quotient, blob proofs, the openings' verifier), then every family's small call again after each of two replacements.  Every
result is checked the way its family's own test checks it -- the host verifiers,
or scalars of the trapdoor oracle -- and must be byte-equal to the same call on a fresh engine.  At the end the engine is
closed and a second one is created, used and closed in the same process."""
import random

import numpy as np
import pytest

import bigint_twin as T
import blob_oracle as BO
import blob_proof_oracle as BP
import cells_oracle as CO
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import lookup_oracle as LO
import ntt_oracle as NO
import perm_quotient_oracle as PQ
import trapdoor_oracle as TO
import verify_openings_oracle as VO

pytestmark = pytest.mark.gpu
R = K.R_MODULUS
S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)
G2 = np.stack([K.srs_g2_at(T.BENCH_SECRET_BE, j) for j in range(17)])


def _poly(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R) for _ in range(n)]


def _points(k, seed):
    return [K.Scalar(v) for v in _poly(k, 9000 + seed)]  # (distinct: k random values below r)


def _values(vals, zs):
    return [K.Scalar(TO.poly_eval(vals, z.v)) for z in zs]


def _raw(points):
    return b"".join(p.p1.tobytes() for p in points)


def _commitments_hold(oracle, commitments, polys):
    return all(c.compress() == TO.commitment(oracle, p, S) for c, p in zip(commitments, polys))


# ---- one call of each family: runs it on e, checks the result when asked to, returns the result's bytes ----------------------
def open_points(k):
    def run(e, oracle, check):
        vals = _poly(40, 100 + k)
        c, zs = K.scalars_to_limbs(vals), _points(k, k)
        ys = _values(vals, zs)
        cm, pi = e.commit_limbs(c), e.open_points_limbs(c, zs, ys)
        if check:
            assert _commitments_hold(oracle, [cm], [vals])
            assert K.verify_points(cm, pi, zs, ys, e.srs_read(0, 16), G2)
        return _raw([cm, pi])
    return run


def open_combined(t, n):
    def run(e, oracle, check):
        polys = [_poly(n, 200 + 1000 * n + i) for i in range(t)]
        a = np.stack([K.scalars_to_limbs(p) for p in polys])
        z, gamma = _points(2, 31 * t + n)
        ys, pi = e.open_combined_limbs(a, z, gamma)
        cms = e.commit_batch_host(a)
        if check:
            assert [y.v for y in ys] == [TO.poly_eval(p, z.v) for p in polys]
            assert _commitments_hold(oracle, cms, polys)
            assert K.verify_combined(cms, ys, z, gamma, pi, G2[1])
        return _raw(cms + [pi]) + b"".join(y.limbs().tobytes() for y in ys)
    return run


def open_sets(nsets):
    def run(e, oracle, check):
        pts = _points(2 * nsets, 70 + nsets)
        # one set of one point, or sets of three points that share one with the next set: 2 * nsets distinct points
        sets = [[pts[0]]] if nsets == 1 else [[pts[2 * g], pts[2 * g + 1], pts[(2 * g + 2) % len(pts)]] for g in range(nsets)]
        set_of = list(range(nsets))
        polys = [_poly(40, 300 + 10 * nsets + i) for i in range(nsets)]
        a = np.stack([K.scalars_to_limbs(p) for p in polys])
        gamma = _points(1, 80 + nsets)[0]
        ys, pi = e.open_sets_limbs(a, set_of, sets, gamma)
        cms = e.commit_batch_host(a)
        if check:
            assert [[y.v for y in row] for row in ys] == [[TO.poly_eval(p, z.v) for z in sets[g]] for p, g in zip(polys, set_of)]
            assert _commitments_hold(oracle, cms, polys)
            assert K.verify_sets(cms, set_of, sets, ys, gamma, pi, e.srs_read(0, 16), G2)
        return _raw(cms + [pi])
    return run


def open_batch(b):
    def run(e, oracle, check):
        if e.max_batch() < b:
            assert e.set_max_batch(b) == b
        polys = [_poly(60, 400 + 10 * b + i) for i in range(b)]
        limbs = [K.scalars_to_limbs(p) for p in polys]
        zs = _points(b, 90 + b)
        ys = [_values(p, [z])[0] for p, z in zip(polys, zs)]
        proofs = e.open_batch_limbs(limbs, zs, ys)
        cms = e.commit_batch_limbs(limbs)
        assert all(isinstance(p, K.G1Point) for p in proofs), proofs
        if check:
            assert _commitments_hold(oracle, cms, polys)
            assert K.verify_proof_batch(cms, proofs, zs, ys, G2[1]) == [True] * b
        return _raw(cms + proofs)
    return run


def _cell_proofs_hold(oracle, proofs, vals, K_, t):
    q = TO.cell_proof_scalars_fast(CO.trim(vals) or [0], K_, t, S)
    return all(p.compress() == TO.g1_scalar(oracle, q[j]) for j, p in enumerate(proofs))


def fk20(t):
    K_, n = 7, 64

    def run(e, oracle, check):
        polys = [_poly(n, 500 + b) for b in range(2)]
        c = np.stack([K.scalars_to_limbs(p) for p in polys])
        cells, proofs = e.cells_and_proofs_fk20(c, K_, t)
        if check:
            l = 1 << t
            for b in range(2):
                assert K.limbs_to_scalars(cells[b]) == CO.cells(polys[b], K_, t), b
                assert _cell_proofs_hold(oracle, proofs[b], polys[b], K_, t), b
            cm, j = e.commit_limbs(c[1]), 5
            zs = [K.Scalar(z) for z in CO.cell_points(K_, t, j)]
            ys = [K.Scalar.from_limbs(v) for v in cells[1][j * l:(j + 1) * l]]
            assert K.verify_points(cm, proofs[1][j], zs, ys, e.srs_read(0, 16), G2)
        return cells.tobytes() + _raw(proofs[0] + proofs[1])
    return run


def recover(K_):
    t = 2

    def run(e, oracle, check):
        N, l = 1 << K_, 1 << t
        n, M = N // 2, N >> t
        polys = [_poly(n, 600 + K_ + b) for b in range(2)]
        cells = [CO.cells(p, K_, t) for p in polys]
        ids = random.Random(K_).sample(range(M), M // 2)
        rx = np.stack([np.stack([K.scalars_to_limbs(cl[j * l:(j + 1) * l]) for j in ids]) for cl in cells])
        co, ce, pr = e.recover_cells_and_proofs(n, K_, t, ids, rx)
        if check:
            for b in range(2):
                assert K.limbs_to_scalars(co[b]) == polys[b], b
                assert K.limbs_to_scalars(ce[b]) == cells[b], b
                assert _cell_proofs_hold(oracle, pr[b], polys[b], K_, t), b
        return co.tobytes() + ce.tobytes() + _raw(pr[0] + pr[1])
    return run


_RECORDS = {}


def _cell_records(oracle):
    """32 valid records (2 polynomials x 16 cells of 8 values) made without the library's device side"""
    if not _RECORDS:
        K_, t, l = 7, 3, 8
        polys = [_poly(64, 700 + b) for b in range(2)]
        _RECORDS["coms"] = [K.G1Point.uncompress(TO.commitment(oracle, p, S)) for p in polys]
        rows = []
        for b, p in enumerate(polys):
            cells = CO.cells(p, K_, t)
            q = TO.cell_proof_scalars_fast(p, K_, t, S)
            for j in range(16):
                rows.append((b, j, K.scalars_to_limbs(cells[j * l:(j + 1) * l]), K.G1Point.uncompress(TO.g1_scalar(oracle, q[j]))))
        random.Random(7).shuffle(rows)
        _RECORDS["rows"] = rows
    return _RECORDS["coms"], _RECORDS["rows"]


def verify_cells(k):
    def run(e, oracle, check):
        coms, rows = _cell_records(oracle)
        idx, ids, vals, prf = zip(*rows[:k])
        ok = e.verify_cells_batch(coms, idx, ids, np.stack(vals), prf, 7, 3, G2[:9])
        wrong = np.stack(vals).copy()
        wrong[k - 1, 3, 0] ^= 1  # another (still canonical) value in the last record
        bad = e.verify_cells_batch(coms, idx, ids, wrong, prf, 7, 3, G2[:9])
        if check:
            assert ok and not bad
        return bytes([ok, bad])
    return run


def blobs(batch):
    n, K_, t = 16, 5, 2

    def run(e, oracle, check):
        rnd = random.Random(800 + batch)
        data = [b"".join(rnd.randrange(R).to_bytes(32, "big") for _ in range(n)) for _ in range(batch)]
        coms, cells, proofs = e.blobs_to_cells_and_proofs_bytes(b"".join(data), n, K_, t)
        if check:
            want = [b"", b"", b""]
            for blob in data:
                c = BO.blob_coefficients(blob, K.KZG_ORDER_NATURAL)
                q = TO.cell_proof_scalars_fast(CO.trim(c) or [0], K_, t, S)
                want[0] += TO.commitment(oracle, c, S)
                want[1] += BO.cells_bytes(c, K_, t, K.KZG_ORDER_NATURAL)
                want[2] += b"".join(TO.g1_scalar(oracle, q[j]) for j in range((1 << K_) >> t))
            assert [coms, cells, proofs] == want
        return coms + cells + proofs
    return run


# ---- the prover families (the SRS holds 2048 points when their large calls run) ---------------------------------------------------
BETA, GAMMA, ALPHA = 0x1F2E3D4C5B6A79881F2E3D4C5B6A7988 % R, 0x123456789ABCDEF0FEDCBA9876543210 % R, 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % R
_MEMO = {}  # inputs and big-integer references, made once


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def _cols(n, t, seed, low=0):
    def make():
        rnd = random.Random(seed)
        return [[rnd.randrange(low, R) for _ in range(n)] for _ in range(t)]
    return _memo(("cols", n, t, seed, low), make)


def _lim(cols):
    return np.stack([GO.to_limbs(c) for c in cols])


def _permutation(k, t, seed):
    def make():
        ks = GO.shifts(t)
        wires, sigmas = GO.true_permutation(k, t, ks, seed)
        z, last = PQ.z_of(wires, sigmas, ks, BETA, GAMMA)
        assert last == 1
        return ks, wires, sigmas, z
    return _memo(("perm", k, t, seed), make)


def grand_product(n, k):
    """kzg_grand_product at n rows (any n), kzg_permutation_commit at 2^k"""
    def run(e, oracle, check):
        nums, dens = _cols(n, 2, 1100 + n), _cols(n, 2, 1200 + n, low=1)
        z, last = e.grand_product_limbs(_lim(nums), _lim(dens))
        ks, wires, sigmas, want_z = _permutation(k, 3, 1300 + k)
        sc = [K.Scalar(x) for x in ks], K.Scalar(BETA), K.Scalar(GAMMA)
        point, pz, plast = e.permutation_commit(_lim(wires), _lim(sigmas), *sc)
        if check:
            assert GO.check(nums, dens, GO.from_limbs(z), GO.from_limbs(last)[0])
            assert GO.from_limbs(pz) == want_z and GO.from_limbs(plast) == [1]
            assert point.compress() == TO.g1_scalar(oracle, NO.barycentric_eval(want_z, S))
        return z.tobytes() + last.tobytes() + _raw([point]) + pz.tobytes() + plast.tobytes()
    return run


def lookup_sums(n):
    def run(e, oracle, check):
        nums, dens = _cols(n, 2, 1400 + n), _cols(n, 2, 1500 + n, low=1)
        phi, last = e.logderivative_sum_limbs(_lim(nums), _lim(dens))
        lookups, table, mult = _memo(("lookup", n), lambda: LO.valid_lookup(n, 2, 1600 + n))
        lphi, llast = e.lookup_sum_limbs(_lim(lookups), GO.to_limbs(table), GO.to_limbs(mult), K.Scalar(BETA))
        if check:
            assert LO.check(nums, dens, GO.from_limbs(phi), GO.from_limbs(last)[0])
            a, b = LO.lookup_columns(lookups, table, mult, BETA)
            assert GO.from_limbs(llast) == [0] and LO.check(a, b, GO.from_limbs(lphi), 0)
        return phi.tobytes() + last.tobytes() + lphi.tobytes() + llast.tobytes()
    return run


def multiplicities(n_table, caps=(None,)):
    """caps: one call per entry, None the default capacity of the hash table, else its log2 (larger than the default's)"""
    def run(e, oracle, check):
        def make():
            rnd = random.Random(1700 + n_table)
            table = list({rnd.randrange(R): None for _ in range(n_table + 8)})[:n_table]
            lookups = [[table[rnd.randrange(n_table)] for _ in range(n_table + 3)] for _ in range(2)]
            return table, lookups, LO.multiplicities(table, lookups)
        table, lookups, (counts, rows, missing) = _memo(("mult", n_table), make)
        out = b""
        for cap in caps:
            mult, got_rows = e.lookup_multiplicities(GO.to_limbs(table), _lim(lookups), log_capacity=cap)
            if check:
                assert missing is None and np.array_equal(mult, GO.to_limbs(counts)) and got_rows.tolist() == rows, cap
            out += mult.tobytes() + got_rows.tobytes()
        return out
    return run


def batch_inverse(n):
    def run(e, oracle, check):
        vals = _cols(n, 1, 1800 + n, low=1)[0]
        out = e.batch_inverse_limbs(GO.to_limbs(vals))
        if check:
            assert all(v * w % R == 1 for v, w in zip(vals, GO.from_limbs(out)))
        return out.tobytes()
    return run


def transforms(n):
    def run(e, oracle, check):
        vals = _cols(n, 1, 1900 + n)[0]
        ev = e.ntt_limbs(GO.to_limbs(vals))
        back = e.intt_limbs(ev)
        if check:
            assert GO.from_limbs(ev) == _memo(("ntt", n), lambda: NO.ntt(vals)) and GO.from_limbs(back) == vals
        return ev.tobytes() + back.tobytes()
    return run


def _evaluation_form(n, seed):
    """(values over the domain, a point outside it, the value there, the coefficients)"""
    def make():
        vals = _cols(n, 1, seed + n)[0]
        z = _poly(1, seed + n + 1)[0]
        return vals, z, NO.barycentric_eval(vals, z), NO.intt(vals)
    return _memo(("evals", n, seed), make)


def evaluations(n):
    def run(e, oracle, check):
        vals, z, y, coef = _evaluation_form(n, 2000)
        a = GO.to_limbs(vals)
        cm, pi = e.commit_evaluations_limbs(a), e.open_evaluations_limbs(a, K.Scalar(z), K.Scalar(y))
        if check:
            assert cm.compress() == TO.commitment(oracle, coef, S) and pi.compress() == TO.proof(oracle, coef, z, S)
            assert K.verify_proof(cm, pi, K.Scalar(z), K.Scalar(y), G2[1])
        return _raw([cm, pi])
    return run


def lagrange(k):
    def run(e, oracle, check):
        vals, z, y, coef = _evaluation_form(1 << k, 2100)
        a = GO.to_limbs(vals)
        e.lagrange_prepare(k)
        cm, pi = e.commit_lagrange_limbs(a), e.open_lagrange_limbs(a, K.Scalar(z), K.Scalar(y))
        if check:
            assert e.lagrange_len() == 1 << k
            assert cm.compress() == TO.commitment(oracle, coef, S) and pi.compress() == TO.proof(oracle, coef, z, S)
        return _raw([cm, pi]) + e.lagrange_read(0, 1 << k).tobytes()
    return run


def coset_extend(length, log_N):
    def run(e, oracle, check):
        cols = _cols(length, 3, 2200 + length)
        got = e.coset_extend_limbs(_lim(cols), log_N)
        if check:
            want = _memo(("ext", length, log_N), lambda: [PQ.coset_extend(NO.intt(c), log_N) for c in cols])
            assert np.array_equal(got, _lim(want))
        return got.tobytes()
    return run


def permutation_quotient(log_ext, t):
    """n = 256; the chunks are committed where the SRS holds them"""
    n = 256

    def run(e, oracle, check):
        ks, wires, sigmas, z = _permutation(8, t, 2300 + t)
        committed = e.srs_len() >= n
        coeffs, points = e.permutation_quotient(_lim(wires), _lim(sigmas), GO.to_limbs(z), [K.Scalar(x) for x in ks], K.Scalar(ALPHA),
                                                K.Scalar(BETA), K.Scalar(GAMMA), log_ext, want_commitments=committed)
        if check:
            T_ = _memo(("T", t), lambda: PQ.quotient(wires, sigmas, z, ks, ALPHA, BETA, GAMMA))
            full = list(T_) + [0] * ((n << log_ext) - n - len(T_))
            assert np.array_equal(coeffs, GO.to_limbs(full))
            for c, point in enumerate(points or []):
                assert point.compress() == TO.g1_scalar(oracle, PQ.horner(full[c * n:(c + 1) * n], S)), c
        return coeffs.tobytes() + _raw(points or [])
    return run


def blob_proofs(batch):
    n = 16

    def run(e, oracle, check):
        rnd = random.Random(2400 + batch)
        data = [b"".join(rnd.randrange(R).to_bytes(32, "big") for _ in range(n)) for _ in range(batch)]
        zs = [rnd.randrange(R) for _ in range(batch)]
        ys, proofs = e.blobs_open_at_bytes(b"".join(data), n, b"".join(z.to_bytes(32, "big") for z in zs))
        coms, blob_proofs_ = e.blobs_to_blob_proofs_bytes(b"".join(data), n)
        if check:
            for b, blob in enumerate(data):
                c = BO.blob_coefficients(blob, K.KZG_ORDER_NATURAL)
                assert (ys[32 * b:32 * b + 32], proofs[48 * b:48 * b + 48]) == BP.open_at(oracle, blob, K.KZG_ORDER_NATURAL, zs[b], S, c), b
                com = BP.commitment(oracle, blob, K.KZG_ORDER_NATURAL, S, c)
                assert coms[48 * b:48 * b + 48] == com, b
                want = BP.open_at(oracle, blob, K.KZG_ORDER_NATURAL, BP.challenge(blob, com), S, c)[1]
                assert blob_proofs_[48 * b:48 * b + 48] == want, b
        return ys + proofs + coms + blob_proofs_
    return run


def verify_openings(k):
    def run(e, oracle, check):
        def make():
            polys = [_poly(40, 2500 + b) for b in range(3)]
            idx = [t % 3 for t in range(24)]
            zs = _poly(24, 2510)
            coms, prfs, ys = VO.trapdoor_records(polys, idx, zs, S)
            point = lambda v: K.G1Point.uncompress(TO.g1_scalar(oracle, v))
            return [point(v) for v in coms], idx, zs, ys, [point(v) for v in prfs]
        coms, idx, zs, ys, prfs = _memo("openings", make)
        sc = lambda vals: [K.Scalar(v) for v in vals]
        ok = e.verify_openings_batch(coms, idx[:k], sc(zs[:k]), sc(ys[:k]), prfs[:k], G2[:2])
        wrong = list(ys[:k])
        wrong[k - 1] = (wrong[k - 1] + 1) % R  # another claimed value in the last record
        bad = e.verify_openings_batch(coms, idx[:k], sc(zs[:k]), sc(wrong), prfs[:k], G2[:2])
        if check:
            assert ok and not bad
        return bytes([ok, bad])
    return run


# every prover family small, large, small.  The quotient keeps n = 256 and changes the extension (and the columns): no workspace
# grows, the cached inverses of Z_H are those of another shape every time.  The multiplicities' large step: the default capacity,
# an explicit larger one (the hash table is made again), the default once more
PROVER_SRS = 2048
PROVER_FAMILIES = [
    [("grand product 4", grand_product(4, 2)), ("grand product 2049", grand_product(2049, 11))],
    [("lookup sums 1", lookup_sums(1)), ("lookup sums 1025", lookup_sums(1025))],
    [("multiplicities 1", multiplicities(1)), ("multiplicities 257", multiplicities(257, (None, 12, None)))],
    [("inverse 1", batch_inverse(1)), ("inverse 1025", batch_inverse(1025))],
    [("ntt 2", transforms(2)), ("ntt 4096", transforms(1 << 12))],
    [("evaluations 4", evaluations(4)), ("evaluations 2048", evaluations(2048))],
    [("lagrange 4", lagrange(2)), ("lagrange 128", lagrange(7))],
    [("extend 8", coset_extend(4, 3)), ("extend 4096", coset_extend(1 << 10, 12))],
    [("quotient e=4", permutation_quotient(2, 3)), ("quotient e=8", permutation_quotient(3, 7))],
    [("blob proofs 1", blob_proofs(1)), ("blob proofs 3", blob_proofs(3))],
    [("openings 2", verify_openings(2)), ("openings 24", verify_openings(24))],
]


# every family small, large, small (the combined openings once with 16 and once with 200 coefficients)
FAMILIES = [
    [("points 2", open_points(2)), ("points 16", open_points(16))],
    [("combined 2x16", open_combined(2, 16)), ("combined 40x16", open_combined(40, 16))],
    [("combined 2x200", open_combined(2, 200)), ("combined 40x200", open_combined(40, 200))],
    [("sets 1", open_sets(1)), ("sets 8", open_sets(8))],
    [("batch 1", open_batch(1)), ("batch 4", open_batch(4))],
    [("fk20 cells of 2", fk20(1)), ("fk20 cells of 8", fk20(3))],
    [("recover 16", recover(4)), ("recover 64", recover(6))],
    [("verify 2", verify_cells(2)), ("verify 24", verify_cells(24))],
    [("blobs 1", blobs(1)), ("blobs 3", blobs(3))],
]
# the first small calls, repeated after each SRS replacement (the combined opening of 200 coefficients needs the longer SRS)
SMALL = [small for small, _ in FAMILIES if small[0] != "combined 2x200"] + [small for small, _ in PROVER_FAMILIES]


def test_buffers_are_created_grown_and_reused(oracle):
    fresh = {}

    def reference(name, run, srs_len):
        """the bytes of the same call on an engine that has done nothing else (made once per call and SRS length)"""
        if (name, srs_len) not in fresh:
            f = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(srs_len)
            try:
                fresh[name, srs_len] = run(f, oracle, False)
            finally:
                f.close()
        return fresh[name, srs_len]

    e = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(256)
    try:
        def step(call, srs_len=256):
            name, run = call
            assert e.srs_len() == srs_len
            assert run(e, oracle, True) == reference(name, run, srs_len), name

        for small, large in FAMILIES:
            step(small)
            step(large)
            step(small)
        e.srs_generate(T.BENCH_SECRET_BE, PROVER_SRS)  # the SRS grows: room for the prover families' large calls
        for small, large in PROVER_FAMILIES:
            step(small, PROVER_SRS)
            step(large, PROVER_SRS)
            step(small, PROVER_SRS)
        for srs_len in (128, 256):  # the grown buffers survive an SRS replacement; the MSM workspaces are made again
            e.srs_generate(T.BENCH_SECRET_BE, srs_len)
            assert e.lagrange_len() == 0  # the Lagrange basis went with the SRS it was made from: the next call builds it again
            for call in SMALL:
                step(call, srs_len)
    finally:
        e.close()
    # destruction leaves the device usable: a second engine in the same process, one commitment, closed again
    second = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(256)
    try:
        vals = _poly(256, 1)
        assert second.commit_limbs(K.scalars_to_limbs(vals)).compress() == TO.commitment(oracle, vals, S)
    finally:
        second.close()
