"""The MSM pipeline at its internal boundaries, checked against the trapdoor oracle [P(s)]G (tests/trapdoor_oracle.py).

Single-digit scalars (v <= 2^(c-1), or r - v for a negated point) put exactly one reference into bucket v - 1, so a list
of bucket populations fixes where the segments of the accumulation (L = accumulate_seg_len(M, lanes)) cut every bucket.
The families of trapdoor_oracle.FAMILIES name the constant each population targets:
  segment_edges   L - 1, L, L + 1, 2L, 2L + 1 references starting at offsets 0, 1, L - 1 of a segment (part_a / part_b)
  tree_threshold  spans of S - 1 .. S + 2 pieces, S = kSerialSpan (16) with many buckets, group_span_limit(group) (64 or
                  more) when several quads share a bucket; 16/17 and kSerialSpanFew 4/5 pieces too
  tree_chunks     spans of 64k - 1, 64k, 64k + 1 and 4096 +- 1 pieces (kChunk pieces per tree, kChunk chunks per group)
  inside_segment  buckets complete inside one segment at every offset, whole-segment-only buckets
  staircase       populations 1, 2, 3, ...
  max_heavy       buckets of S + 1 pieces owning S - 1 segments each, back to back (kMaxEntries / kMaxChunks1/2 bound)
  first_last      bucket 0, a run of empty buckets, the last bucket with every other reference
(kSerialSpanFew only applies to k_bucket_finalize, which the library runs when nb > 8192 buckets, i.e. never with few
buckets: finalize_group_size gives those several quads per bucket.)
Every case also checks the device's reference count (KernelTimes.references) against the recoding model's M."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import bigint_twin as T
import kzg_poly_commit_exploration_amd as K
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu

R = TO.R
BENCH_S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)
N16 = (1 << 16) + 1
N20 = (1 << 20) + 1
N22 = (1 << 22) + 1
OMEGA3 = pow(7, (R - 1) // 3, R)  # a primitive cube root of unity: SRS[i] = SRS[i mod 3]
HERE = os.path.dirname(os.path.abspath(__file__))


def limbs_of(vals):
    """Montgomery limbs; repeated values are converted once (structured inputs have few distinct values)"""
    distinct = {}
    idx = np.fromiter((distinct.setdefault(v % R, len(distinct)) for v in vals), dtype=np.int64, count=len(vals))
    table = K.scalars_to_limbs(list(distinct))
    return np.ascontiguousarray(table[idx])


def commit_with_refs(eng, limbs):
    """(compressed commitment, references counted by the device) through slot 0 with timing on"""
    dptr = eng.dev_alloc(limbs.nbytes)
    try:
        eng.dev_upload(dptr, limbs)
        eng.set_timing(True)
        eng.commit_submit(0, dptr, limbs.shape[0])
        got = eng.wait(0).compress()
        refs = eng.times(0)["references"]
    finally:
        eng.set_timing(False)
        eng.dev_free(dptr)
    return got, refs


def check_values(oracle, eng, s, vals, c, label, refs=True):
    got, dev_refs = commit_with_refs(eng, limbs_of(vals))
    assert got == TO.commitment(oracle, vals, s), label
    if refs and not any(TO.near_fold_boundary(v) for v in vals):
        assert dev_refs == TO.count_refs(vals, c), label


def check_family(oracle, eng, s, job, family, seed=0):
    M = job.n
    pops, placed, L, S = TO.family_layout(family, job, M)
    assert placed, family
    vals = TO.values_from_pops(pops, random.Random(seed))
    got, dev_refs = commit_with_refs(eng, limbs_of(vals))
    where = "%s, L=%d, S=%d, %d cases, first %s" % (family, L, S, len(placed), next(iter(placed)))
    assert got == TO.commitment(oracle, vals, s), where
    assert dev_refs == M, where  # one reference per single-digit scalar
    return placed


# ---------------------------------------------------------------- §2 accumulation, finalisation and trees


@pytest.mark.parametrize("family", sorted(TO.FAMILIES))
def test_boundaries_small_msm(engines, oracle, family):
    """k_small_msm with its accumulation phase: 2501 terms at 10-bit windows, 26 x 2501 <= kTinyRefs, L = 4"""
    eng = engines.bench_srs(2501)
    job = TO.Job(2501, 2501)
    assert job.small and not job.direct and (job.c, job.nb) == tuple(eng.msm_config()[k] for k in ("digit_bits", "buckets"))
    check_family(oracle, eng, BENCH_S, job, family)


def test_small_msm_direct_form_edges(oracle):
    """launch_small_msm's direct form (max_refs <= nb * 32: no accumulation phase) and the first size past it; one bucket
    with more than kDirectGroupRefs references goes to a whole workgroup (every digit of a scalar equal)"""
    eng = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(1024)
    try:
        c, W, nb, _ = TO.msm_config(1024)
        assert eng.msm_config()["digit_bits"] == c == 8
        direct_max = nb * 32 // W  # 128 terms
        rng = random.Random(5)
        for n in (101, 102, direct_max, direct_max + 1):
            job = TO.Job(1024, n)
            assert job.small and job.direct == (n <= direct_max)
            check_values(oracle, eng, BENCH_S, [TO.bucket_value(i % nb, i % 3 == 0) for i in range(n)], c, "ramp n=%d" % n)
            check_values(oracle, eng, BENCH_S, TO.values_from_pops([n] + [0] * (nb - 1), rng), c, "one bucket n=%d" % n)
            every = sum(5 << (c * j) for j in range(W - 1))  # digit 5 in every window but the top one
            check_values(oracle, eng, BENCH_S, [every] * n, c, "kDirectGroupRefs n=%d" % n)
            check_values(oracle, eng, BENCH_S, [rng.randrange(R) for _ in range(n)], c, "uniform n=%d" % n)
    finally:
        eng.close()


@pytest.mark.parametrize("family", sorted(TO.FAMILIES))
def test_boundaries_general_2_16(engines, oracle, family):
    """general kernels, 2^16 + 1 terms: 13-bit windows, 4096 buckets of 4 quads, L = 8, S = 64"""
    eng = engines.bench_srs(N16)
    job = TO.Job(N16, N16)
    assert not job.small and eng.msm_config()["digit_bits"] == job.c
    check_family(oracle, eng, BENCH_S, job, family)


@pytest.mark.parametrize("family", sorted(TO.FAMILIES))
def test_boundaries_general_2_20(engines, oracle, family):
    """general kernels, 2^20 + 1 terms: 17-bit windows, 65536 buckets (k_bucket_finalize), L = 9, S = kSerialSpan"""
    eng = engines.bench_srs(N20)
    job = TO.Job(N20, N20)
    assert TO.tree_span_limit(job.nb) == TO.K_SERIAL_SPAN and job.L(N20) == 9
    placed = check_family(oracle, eng, BENCH_S, job, family, seed=20)
    if family == "max_heavy":
        assert len(placed) > 7000


CHILD = r"""
import json, os, random, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "oracle"), %(tests)r]
import bigint_twin as T, kzg_poly_commit_exploration_amd as K, oracle_ctypes as O, trapdoor_oracle as TO
import test_msm_boundaries_gpu as B
O.lib()
n, mode = %(n)d, %(mode)r
forced = int(os.environ["KZG_MSM_C"]) if "KZG_MSM_C" in os.environ else None
lanes = int(os.environ.get("KZG_ACCUM_LANES", TO.K_DEFAULT_LANES))
s = B.BENCH_S
bad = []
widths = range(8, 21) if mode == "widths" else [forced]
for c in widths:
    if mode == "widths":
        os.environ["KZG_MSM_C"] = str(c)  # read when the SRS is sized: one engine per width
    eng = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(n)
    try:
        job = TO.Job(n, n, forced_c=c, lanes_target=lanes)
        if eng.msm_config()["digit_bits"] != job.c:
            bad.append(["config", eng.msm_config(), job.c])
            continue
        if mode in ("families", "widths"):
            for fam in (sorted(TO.FAMILIES) if mode == "families" else ["staircase", "first_last"]):
                try:
                    B.check_family(O, eng, s, job, fam)
                except AssertionError as e:
                    bad.append([c, fam, str(e)[:300]])
        if mode in ("recoding", "widths"):
            rng = random.Random(c or 0)
            fam = TO.recoding_family(job.c)
            vals = (fam * (n // len(fam) + 1))[:n]
            rng.shuffle(vals)
            try:
                B.check_values(O, eng, s, vals, job.c, "recoding family c=%%d" %% job.c)
                clean = [v for v in fam if not TO.near_fold_boundary(v)]
                B.check_values(O, eng, s, (clean * (n // len(clean) + 1))[:n], job.c, "recoding clean c=%%d" %% job.c)
            except AssertionError as e:
                bad.append([c, "recoding", str(e)[:300]])
    finally:
        eng.close()
print(json.dumps({"bad": bad}))
"""


def run_child(env_extra, n, mode, timeout):
    root = os.path.dirname(HERE)
    script = CHILD % {"root": root, "tests": HERE, "n": n, "mode": mode}
    env = dict(os.environ, **env_extra)
    p = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=timeout, env=env)
    assert p.returncode == 0, (env_extra, p.stdout[-2000:], p.stderr[-3000:])
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["bad"] == [], (env_extra, res["bad"])


@pytest.mark.parametrize("env", [{"KZG_ACCUM_LANES": "4096"}, {"KZG_ACCUM_LANES": "1000"}, {"KZG_MSM_C": "12"}],
                         ids=["lanes4096", "lanes1000", "c12"])
def test_boundaries_under_other_knobs(env):
    """the same families at 2^16 + 1 in a child process (the switches are read once per process): few lanes make the
    segments long (L = 17 at 4096 lanes, 65 at 1024 -- KZG_ACCUM_LANES=1000 rounds up to 1024), so the spans land at other
    offsets; KZG_MSM_C=12 gives 2048 buckets (= kFewBuckets) and 22 windows"""
    run_child(env, N16, "families", 900)


# ---------------------------------------------------------------- §3 recoding edges on every sort kernel


def test_recoding_edges_k_sort_small(engines, oracle):
    """k_sort_small (one polynomial, n <= 4096): the recoding family at 10-bit windows"""
    eng = engines.bench_srs(2501)
    c = eng.msm_config()["digit_bits"]
    fam = TO.recoding_family(c)
    rng = random.Random(3)
    vals = (fam * (2501 // len(fam) + 1))[:2501]
    rng.shuffle(vals)
    check_values(oracle, eng, BENCH_S, vals, c, "family")
    clean = [v for v in fam if not TO.near_fold_boundary(v)]
    check_values(oracle, eng, BENCH_S, clean, c, "clean family")  # short polynomial, counted references
    check_values(oracle, eng, BENCH_S, fam[:3], c, "0, 1, r - 1")


def test_recoding_edges_count_and_staged_spread(engines, oracle):
    """k_sort_count + k_sort_spread_staged (packed pairs) at 2^16 + 1"""
    eng = engines.bench_srs(N16)
    c = eng.msm_config()["digit_bits"]
    fam = TO.recoding_family(c)
    clean = [v for v in fam if not TO.near_fold_boundary(v)]
    rng = random.Random(4)
    for src, label in ((fam, "family"), (clean, "clean family")):
        vals = (src * (N16 // len(src) + 1))[:N16]
        rng.shuffle(vals)
        check_values(oracle, eng, BENCH_S, vals, c, label)


def test_recoding_edges_unpacked_pairs():
    """k_sort_spread with 8-byte pairs (KZG_SORT_PACKED=0), the form degree 2^22 and batches of 8 at 2^20 take"""
    run_child({"KZG_SORT_PACKED": "0"}, N16, "recoding", 900)
    run_child({"KZG_SORT_PACKED": "0"}, N16, "families", 900)


def test_recoding_every_forced_width():
    """KZG_MSM_C = 8 .. 20 at 600 points, the widths the chooser skips (top window of 1-3 bits) included"""
    run_child({}, 600, "widths", 900)


# ---------------------------------------------------------------- §4 production shapes at full size

_inputs = {}


def full_size_polys(n):
    """distinct structured polynomials of n terms as (label, values, limbs), built once per module"""
    if n in _inputs:
        return _inputs[n]
    rng = random.Random(n)
    out = []
    bench = T.bench_coefficients(n - 1)
    bench += [0] * (n - len(bench))
    out.append(("bench", bench))
    out.append(("zero", [0] * n))
    out.append(("all ones", [1] * n))
    out.append(("0/1", [rng.getrandbits(1) for _ in range(n)]))
    job = TO.Job(n, n)
    pops, _, _, _ = TO.family_layout("staircase", job, n)
    out.append(("staircase", TO.values_from_pops(pops, rng)))
    out.append(("i128", [T.fr_from_i128(rng.randrange(-(1 << 127), 1 << 127)) for _ in range(n)]))
    out.append(("near r", [R - 1 - rng.randrange(1 << 20) for _ in range(n)]))
    out.append(("uniform", [rng.randrange(R) for _ in range(n)]))
    _inputs[n] = [(label, vals, limbs_of(vals)) for label, vals in out]
    return _inputs[n]


def test_batch_of_eight_distinct_polynomials_2_20(engines, oracle):
    """8 distinct polynomials of 2^20 + 1 terms in one batch: 8 x 65536 buckets -> the unpacked sort; 4 of them: the
    packed form with a batch.  The zero and one-bucket polynomials sit next to uniform ones, so a batch that reads or
    writes another polynomial's scalars, bucket ids or results gives a wrong commitment in some slot."""
    eng = engines.bench_srs(N20)
    polys = full_size_polys(N20)
    want = {label: TO.commitment(oracle, vals, BENCH_S) for label, vals, _ in polys}
    before = eng.max_batch()
    try:
        assert eng.set_max_batch(8) == 8
        order = [0, 7, 1, 6, 2, 5, 3, 4]  # bench, uniform, zero, near r, all ones, i128, 0/1, staircase
        got = eng.commit_batch_limbs([polys[i][2] for i in order])
        assert [g.compress() for g in got] == [want[polys[i][0]] for i in order]
        four = [1, 7, 4, 2]  # zero, uniform, staircase, all ones
        got = eng.commit_batch_limbs([polys[i][2] for i in four])
        assert [g.compress() for g in got] == [want[polys[i][0]] for i in four]
        # openings of distinct polynomials at distinct points
        rng = random.Random(8)
        zs = [rng.randrange(R) for _ in order]
        ys = [TO.poly_eval(polys[i][1], z) for i, z in zip(order, zs)]
        got = eng.open_batch_limbs([polys[i][2] for i in order], [K.Scalar(z) for z in zs], [K.Scalar(y) for y in ys])
        for j, i in enumerate(order):
            label, vals, _ = polys[i]
            if label == "zero":
                assert got[j].compress() == TO.g1_scalar(oracle, 0)
                continue
            assert got[j].compress() == TO.proof(oracle, vals, zs[j], BENCH_S, ys[j]), label
    finally:
        eng.set_max_batch(before)


def test_degree_2_22_skewed_commitment_and_opening(oracle):
    """2^22 + 1 terms: unpacked sort, 262144 buckets; an all-ones polynomial puts every reference into bucket 0 (the
    heavy trees at the largest size) and a staircase spreads boundaries over all offsets"""
    eng = K.SetupArtifactsGenerator(T.BENCH_SECRET_BE).take(N22)
    try:
        ones = np.ascontiguousarray(np.tile(K.scalars_to_limbs([1]), (N22, 1)))
        want = TO.g1_scalar(oracle, (pow(BENCH_S, N22, R) - 1) * pow(BENCH_S - 1, R - 2, R))  # sum of s^i, i < N22
        assert eng.commit_limbs(ones).compress() == want
        z = 0x5EED
        y = (pow(z, N22, R) - 1) * pow(z - 1, R - 2, R) % R
        assert eng.open_limbs(ones, K.Scalar(z), K.Scalar(y)).compress() == TO.proof(oracle, [1] * N22, z, BENCH_S, y)
        job = TO.Job(N22, N22)
        pops, _, _, _ = TO.family_layout("staircase", job, N22)
        vals = TO.values_from_pops(pops, random.Random(22))
        assert eng.commit_limbs(limbs_of(vals)).compress() == TO.commitment(oracle, vals, BENCH_S)
    finally:
        eng.close()


# ---------------------------------------------------------------- §5 degenerate and colliding trusted setups


def _setup_cases(n, c):
    rng = random.Random(c)
    W = TO.windows_of(c)
    pops, _, _, _ = TO.family_layout("staircase", TO.Job(n, n), n)
    return [("equal", [12345] * n),
            ("single digit", TO.values_from_pops(pops, rng)),
            ("all digits 1", [sum(1 << (c * j) for j in range(W) if c * j < 254) % R] * n),
            ("uniform", [rng.randrange(R) for _ in range(n)])]


@pytest.mark.parametrize("secret", [0, 1, R - 1, 2, OMEGA3], ids=["s=0", "s=1", "s=r-1", "s=2", "s=omega3"])
def test_degenerate_secrets_default_kernels_2_16(oracle, secret):
    """equal points (s = 1), infinities (s = 0), opposite points (s = -1), SRS[i] = SRS[i mod 3] (s = cube root of unity),
    table levels that coincide with other points (s = 2): the equal-point and opposite-point branches of the mixed
    addition and of xyzz30_add_quad in the finalisation and reduction trees, at the default knobs"""
    if secret == OMEGA3:
        assert secret != 1 and pow(secret, 3, R) == 1
    eng = K.SetupArtifactsGenerator(TO.secret_be(secret)).take(N16)
    try:
        c = eng.msm_config()["digit_bits"]
        for label, vals in _setup_cases(N16, c):
            got, _ = commit_with_refs(eng, limbs_of(vals))
            assert got == TO.commitment(oracle, vals, secret), label
    finally:
        eng.close()


@pytest.mark.parametrize("secret", [1, R - 1], ids=["s=1", "s=r-1"])
def test_degenerate_secrets_default_kernels_2_20(oracle, secret):
    eng = K.SetupArtifactsGenerator(TO.secret_be(secret)).take(N20)
    try:
        c = eng.msm_config()["digit_bits"]
        for label, vals in _setup_cases(N20, c):
            got, _ = commit_with_refs(eng, limbs_of(vals))
            assert got == TO.commitment(oracle, vals, secret), label
    finally:
        eng.close()
