"""The false positive of the one-word zero pre-test through k_bucket_accumulate itself (msm_accum.hip): fq_maybe_zero(P) true,
fq_is_zero(P) false, accum_rare_call returns true, and acc, P and Rn come back from private memory for xyzz30_acc_tail.  It
happens to 7 x 2^-30 of all additions; every other test that enters the call does so with equal or opposite operands,
where the call returns false.

What guarantees that the path is taken here, without a counter in the kernel:
  * the SRS is loaded with kzg_srs_load_affine, whose table digits are fq_mul(fq_from_u32x12(w), fq_one()): the g++ build of
    the same two calls gives the same digits bit for bit (tests/accum_false_positives.py);
  * every coefficient is a single-digit scalar, so the sorted references are known (tests/trapdoor_oracle.py), and each pair
    found by the host search sits alone in a bucket of two inside one lane's segment: the first reference finds the
    accumulator at infinity (xyzz30_acc_set: ZZ = fq_one_cold()), the second meets exactly the head the host model ran --
    in either order of arrival and under either sign, since the pre-test reads x only;
  * the mutation run recorded in DESIGN.md section 4.2a: a kernel that forces `more` to false behind accum_rare_call, or an
    xyzz30_acc_rare that returns false on a false positive, fails these tests (and, the former, nothing else).
The rows are k G, k = 1 .. 65537, plus four repeated rows so that true doubling and cancellation exist on the same SRS;
expected commitments are [sum c_i k_i] G from the oracle's scalar multiplication."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import accum_false_positives as FP
import kzg_poly_commit_exploration_amd as K
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = TO.R
DUP_OF = (10, 11, 12, 13)  # rows N_ROWS + d repeat row DUP_OF[d]


class Setup:
    def __init__(self, tmp):
        out = os.path.join(tmp, "libf30f.so")
        subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "host", "field30_fused_host.cpp")],
                       check=True)
        lib = ctypes.CDLL(out)
        pts = FP.multiples_of_g(FP.N_ROWS)
        rows = FP.affine_rows(pts)
        self.pairs = FP.false_positive_pairs(lib, FP.table_digits(lib, rows))  # found now, by the host model
        assert len(self.pairs) >= 4, self.pairs
        self.k = [i + 1 for i in range(FP.N_ROWS)] + [d + 1 for d in DUP_OF]  # row i is [k[i]] G
        self.n = len(self.k)
        self.job = TO.Job(self.n, self.n)
        self.eng = K.Engine()
        self.eng.srs_load_affine(np.concatenate([rows, rows[list(DUP_OF)]]))


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    s = Setup(str(tmp_path_factory.mktemp("accum_fp")))
    yield s
    s.eng.close()


def plan_pairs(s, L):
    """every pair in a bucket of two, back to back from reference 0 (two references never straddle a segment: L is even or
    the model below says no), then a doubling and a cancellation"""
    buckets = [("false positive", [i, j]) for i, j in s.pairs]
    buckets.append(("doubling", [DUP_OF[0], FP.N_ROWS + 0]))
    buckets.append(("cancellation", [DUP_OF[1], FP.N_ROWS + 1]))
    return buckets


def plan_one_wave(s, L):
    """lane l of the first wave owns references [l L, l L + L).  In iteration 1 lane 0 meets a false positive, lane 1 a
    doubling, lane 2 a cancellation, lane 3 the first point of a run, lane 4 a plain addition, lanes 5.. the other false
    positives, another doubling and cancellation, then plain additions up to lane 63"""
    free = iter(range(100, 40000))  # rows for the fillers (none of them a pair's: checked by the caller)
    used = {r for p in s.pairs for r in p} | set(DUP_OF)

    def fill(count):
        out = []
        while len(out) < count:
            r = next(free)
            if r not in used:
                out.append(r)
        return out
    lanes = [("false positive", list(s.pairs[0])), ("doubling", [DUP_OF[0], FP.N_ROWS + 0]),
             ("cancellation", [DUP_OF[1], FP.N_ROWS + 1]), ("first point", fill(1)), ("plain", fill(L))]
    lanes += [("false positive", list(p)) for p in s.pairs[1:]]
    lanes += [("doubling", [DUP_OF[2], FP.N_ROWS + 2]), ("cancellation", [DUP_OF[3], FP.N_ROWS + 3])]
    lanes += [("plain", fill(L)) for _ in range(64 - len(lanes))]
    buckets = []
    for kind, refs in lanes:
        buckets.append((kind, refs))
        if len(refs) < L:
            buckets.append(("filler", fill(L - len(refs))))
    return buckets


def coefficients(s, buckets, signs, rng):
    """one single-digit scalar per row: bucket b holds the rows of buckets[b], the rest of the rows go to the buckets
    behind them.  signs: 0 = every scalar positive, 1 = every scalar negative, 2 = drawn per row (a cancellation bucket
    always gets opposite signs, a doubling bucket equal ones).  -> (values, sum c_i k_i, bucket populations)"""
    assert len(buckets) < s.job.nb - 64
    vals, pops = [None] * s.n, [0] * s.job.nb
    for b, (kind, refs) in enumerate(buckets):
        neg = [signs == 1 if signs < 2 else bool(rng.randrange(2)) for _ in refs]
        if kind == "cancellation":
            neg[1] = not neg[0]
        if kind == "doubling":
            neg[1] = neg[0]
        for r, ng in zip(refs, neg):
            assert vals[r] is None
            vals[r] = TO.bucket_value(b, ng)
        pops[b] = len(refs)
    rest = [r for r in range(s.n) if vals[r] is None]
    first = len(buckets)
    for t, r in enumerate(rest):
        b = first + t % (s.job.nb - first)
        vals[r] = TO.bucket_value(b, signs == 1 if signs < 2 else bool(rng.randrange(2)))
        pops[b] += 1
    total = sum((v if v <= TO.HALF else v - R) * k for v, k in zip(vals, s.k)) % R
    return vals, total, pops


def iteration_one(buckets, pops, L):
    """what lane l < 64 meets in loop iteration 1 (its second reference), from the model of the sorted references"""
    start, at = [], 0
    for p in pops:
        start.append(at)
        at += p
    owner = {}
    for b, (kind, refs) in enumerate(buckets):
        for e in range(start[b], start[b] + len(refs)):
            owner[e] = (b, kind)
    met = []
    for lane in range(64):
        e = lane * L + 1
        b, kind = owner[e]
        if start[b] == e:
            met.append("first point")
        elif start[b] == e - 1 and len(buckets[b][1]) == 2:
            met.append(kind)  # the second of a bucket of two whose first one set the accumulator
        else:
            met.append("plain")
    return met


@pytest.mark.parametrize("plan", [plan_pairs, plan_one_wave], ids=["pairs_back_to_back", "one_wave_every_case"])
def test_false_positive_pairs_through_the_accumulation_kernel(oracle, setup, plan):
    s = setup
    job = s.job
    assert not job.small and job.max_refs > TO.K_TINY_REFS  # the general kernels
    assert s.eng.msm_config()["digit_bits"] == job.c
    M = s.n  # every coefficient is a non-zero single-digit scalar: one reference each
    L = job.L(M)
    assert L >= 4
    buckets = plan(s, L)
    rng = random.Random(1700)
    for signs in (0, 1, 2):
        vals, total, pops = coefficients(s, buckets, signs, rng)
        assert all(1 <= (v if v <= TO.HALF else R - v) <= job.nb for v in vals) and sum(pops) == M
        # from the model: each bucket of two lies inside one lane's segment, right behind the end of another bucket
        at = 0
        for (kind, refs), p in zip(buckets, pops):
            assert p == len(refs)
            if len(refs) == 2:
                assert at // L == (at + 1) // L, (kind, at)
            at += p
        if plan is plan_one_wave:
            met = iteration_one(buckets, pops, L)
            assert met[:5] == ["false positive", "doubling", "cancellation", "first point", "plain"]
            assert met.count("false positive") == len(s.pairs) and met.count("doubling") == 2 and met.count("cancellation") == 2
        distinct = sorted(set(vals))  # (each value is converted once)
        where = {v: t for t, v in enumerate(distinct)}
        limbs = np.ascontiguousarray(K.scalars_to_limbs(distinct)[[where[v] for v in vals]])
        assert s.eng.commit_limbs(limbs).compress() == TO.g1_scalar(oracle, total), "signs %d" % signs
