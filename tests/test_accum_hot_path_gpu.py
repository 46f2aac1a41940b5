"""k_bucket_accumulate's mixed addition (xyzz30_acc_head / accum_rare_call / xyzz30_acc_tail, msm_accum.hip) through the
general kernels, not k_small_msm: 4400 terms are more than kTinyRefs = 65536 references.  Degenerate trusted setups make every
lane meet the out-of-line cases -- s = 0: every point but the first at infinity; s = 1: every point equal (doubling);
s = r - 1: points alternate between G and -G (cancellation, and doubling of the negated point) -- and the coefficient vectors
decide what shares a bucket.  48-byte commitments against the trapdoor oracle [P(s)]G (tests/trapdoor_oracle.py)."""
import random

import numpy as np
import pytest

import bigint_twin as T
import kzg_poly_commit_exploration_amd as K
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu

R = TO.R
N = 4400
GOLDEN_S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)


def limbs_of(vals):
    """Montgomery limbs; repeated values are converted once"""
    distinct = {}
    idx = np.fromiter((distinct.setdefault(v % R, len(distinct)) for v in vals), dtype=np.int64, count=len(vals))
    return np.ascontiguousarray(K.scalars_to_limbs(list(distinct))[idx])


def coefficient_vectors():
    rng = random.Random(4400)
    c = rng.randrange(1, R)
    return [("all equal", [c] * N),
            ("alternating c, -c", [c if i % 2 == 0 else R - c for i in range(N)]),
            ("half zeros", [0 if i % 2 else rng.randrange(1, R) for i in range(N)]),
            ("pseudo-random", [rng.randrange(R) for _ in range(N)])]


@pytest.mark.parametrize("secret", [0, 1, R - 1, GOLDEN_S], ids=["s=0", "s=1", "s=r-1", "s=golden"])
def test_general_accumulation_meets_every_case_of_the_addition(oracle, secret):
    job = TO.Job(N, N)
    assert not job.small and job.max_refs > TO.K_TINY_REFS  # the general kernels
    eng = K.SetupArtifactsGenerator(TO.secret_be(secret)).take(N)
    try:
        assert eng.msm_config()["digit_bits"] == job.c
        for label, vals in coefficient_vectors():
            assert eng.commit_limbs(limbs_of(vals)).compress() == TO.commitment(oracle, vals, secret), label
    finally:
        eng.close()
