"""CPU: the arithmetic of the multilinear kernels (csrc/multilinear_kernels.hip) replayed on the host at the magnitudes their bound
comments allow (tests/host/ml_reach_host.cpp: a stand-alone program built with g++, nothing is loaded into this process): values
r - 1, (r - 1) / 2 and 0, and u, r, gamma in {1, r - 1, (r +- 1) / 2}.  Every result is compared with the Python integer, the digit,
top-digit and column extremes with the bounds the comments state."""
import itertools
import os
import subprocess

import pytest

import multilinear_oracle as MO

R = MO.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M256 = (1 << 256) % R
HALF = (R - 1) // 2
VALUES = (R - 1, HALF, 0)
MULTS = (1, R - 1, (R + 1) // 2, (R - 1) // 2)
# the bounds of the comments: a raw difference of two carry-normalised values (ml_fold1), a carry-normalised digit, the top digit
# of a sum of 256 products (kR9SumTopBound), a product column
RAW_BOUND, NORM_BOUND, TOP_BOUND, COLUMN_BOUND = (1 << 30) + 8, (1 << 29) + 4, 1 << 22, 1 << 63
TOP_R = R >> 240  # the top digit of r


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ml") / "ml_reach")
    # -fwrapv: a digit sum that overflowed would wrap on the device, and so must it here
    subprocess.run(["g++", "-O2", "-fwrapv", "-o", exe, os.path.join(ROOT, "tests", "host", "ml_reach_host.cpp")], check=True)

    def run(head, images, mults):
        text = head + "\n" + " ".join("%064x" % (v % R) for v in images) + "\n" + " ".join("%064x" % (m * M256 % R) for m in mults) + "\n"
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
        return [int(v) for v in out[:4]], [int(v, 16) for v in out[4:]]

    return run


def _in_bounds(rep):
    return rep[0] <= RAW_BOUND and rep[1] <= NORM_BOUND and rep[2] < TOP_BOUND and rep[3] < COLUMN_BOUND


def test_fold_chain_stays_canonical(replay):
    """eleven chained folds (one launch of k_ml_fold): the value is canonical after every fold, so no digit grows along the chain --
    the top digit never passes 1.5002 r + 1, whatever u and the leaves are"""
    worst = [0, 0, 0, 0]
    for leaves in [(a, b) for a in VALUES for b in VALUES] + [(R - 1, 0, HALF, 1)]:
        for pattern in itertools.product(MULTS, repeat=2):
            us = [pattern[i % 2] for i in range(11)]
            rep, (v,) = replay("fold 11 %d" % len(leaves), leaves, us)
            f = [leaves[j % len(leaves)] for j in range(1 << 11)]
            assert v == MO.folds(f, us)[-1][0], (leaves, pattern)
            assert _in_bounds(rep) and rep[2] <= 1.5002 * TOP_R + 1, (leaves, pattern, rep)
            worst = [max(a, b) for a, b in zip(worst, rep)]
    print("fold: raw %.4f x 2^30, norm %.4f x 2^29, top %d (%.3f r), column %.3f x 2^63" % (
        worst[0] / 2.0**30, worst[1] / 2.0**29, worst[2], worst[2] / TOP_R, worst[3] / 2.0**63))
    assert worst[2] >= 0.99 * TOP_R  # the families reach a full r in the raw sum


def test_eval_accumulators(replay):
    """k_ml_eval: the Horner chain, the lane's product, the signed copy and the sum of 256 lanes"""
    worst = [0, 0, 0, 0]
    for coeffs in [(R - 1,), (HALF,), (R - 1, 0), (0, R - 1), (R - 1, HALF, 0)]:
        for z256, zt in itertools.product(MULTS, repeat=2):
            rep, (s, alt) = replay("eval %d" % len(coeffs), coeffs, [z256, zt])
            lanes = [sum(coeffs[(t + 256 * m) % len(coeffs)] * pow(z256, m, R) for m in range(8)) * zt % R for t in range(256)]
            assert s == sum(lanes) % R and alt == sum(-x if t & 1 else x for t, x in enumerate(lanes)) % R, (coeffs, z256, zt)
            assert _in_bounds(rep), (coeffs, z256, zt, rep)
            worst = [max(a, b) for a, b in zip(worst, rep)]
    print("eval: raw %.4f x 2^30, norm %.4f x 2^29, top %d (%.3f r), column %.3f x 2^63" % (
        worst[0] / 2.0**30, worst[1] / 2.0**29, worst[2], worst[2] / TOP_R, worst[3] / 2.0**63))
    assert worst[2] <= 128.1 * TOP_R + 1  # "below 128.1 r"


def test_combine_sum_of_22_terms(replay):
    """k_ml_combine: a canonical value and 21 products, a carry pass after each"""
    worst = [0, 0, 0, 0]
    for vals in [(R - 1,), (HALF,), (R - 1, 0), (R - 1, HALF)]:
        for g in MULTS:
            gs = [pow(g, i, R) for i in range(22)]
            rep, (f,) = replay("combine 22 %d" % len(vals), vals, gs)
            assert f == sum(vals[i % len(vals)] * gs[i] for i in range(22)) % R, (vals, g)
            assert _in_bounds(rep), (vals, g, rep)
            worst = [max(a, b) for a, b in zip(worst, rep)]
    print("combine: raw %.4f x 2^30, norm %.4f x 2^29, top %d (%.3f r), column %.3f x 2^63" % (
        worst[0] / 2.0**30, worst[1] / 2.0**29, worst[2], worst[2] / TOP_R, worst[3] / 2.0**63))
    assert worst[2] <= 11.6 * TOP_R + 1 and worst[2] < 1 << 19  # "below 11.6 r, its top digit below 2^19"
