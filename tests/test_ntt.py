"""CPU: the NTT references of tests/ntt_oracle.py against the definition, and the library's host-side domain root."""
import random

import pytest

import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import trapdoor_oracle as TO

R = NO.R


def test_modulus_and_two_adicity():
    assert R == K.R_MODULUS
    assert (R - 1) % (1 << 32) == 0 and ((R - 1) >> 32) % 2 == 1


@pytest.mark.parametrize("k", list(range(0, 33)))
def test_root_properties(k):
    w = NO.domain_root(k)
    n = 1 << k
    assert pow(w, n, R) == 1
    if k:
        assert pow(w, n // 2, R) == R - 1  # primitive: w^(n/2) != 1
    if k < 32:
        assert pow(NO.domain_root(k + 1), 2, R) == w  # the domains nest: w_2n^2 = w_n


@pytest.mark.parametrize("k", [0, 1, 2, 5, 16, 22, 32])
def test_library_domain_root(k):
    assert K.domain_root(k).v == NO.domain_root(k)


def test_library_domain_root_refuses_beyond_two_adicity():
    with pytest.raises(K.KzgError) as ei:
        K.domain_root(33)
    assert ei.value.status == K.KZG_ERR_INVALID_ARG


@pytest.mark.parametrize("k", list(range(0, 7)))
def test_oracle_against_definition(k):
    rnd = random.Random(k)
    c = [rnd.randrange(R) for _ in range(1 << k)]
    assert NO.ntt(c) == NO.dft(c)
    assert NO.intt(c) == NO.dft(c, inverse=True)


@pytest.mark.parametrize("k", [0, 1, 3, 8, 12])
def test_round_trip(k):
    rnd = random.Random(100 + k)
    c = [rnd.randrange(R) for _ in range(1 << k)]
    assert NO.intt(NO.ntt(c)) == c
    assert NO.ntt(NO.intt(c)) == c


def test_special_inputs():
    n = 64
    assert NO.ntt([0] * n) == [0] * n
    assert NO.ntt([5] + [0] * (n - 1)) == [5] * n  # constant polynomial
    assert NO.intt([9] * n) == [9] + [0] * (n - 1)  # constant values: one-hot coefficients
    w = NO.domain_root(6)
    assert NO.ntt([0] * (n - 1) + [1]) == [pow(w, (n - 1) * i, R) for i in range(n)]


@pytest.mark.parametrize("k", [0, 1, 4, 10])
def test_barycentric_matches_interpolated_coefficients(k):
    rnd = random.Random(200 + k)
    e = [rnd.randrange(R) for _ in range(1 << k)]
    c = NO.intt(e)
    for s in (rnd.randrange(R), 2, R - 1):
        assert NO.barycentric_eval(e, s) == TO.poly_eval(c, s)
    w = NO.domain_root(k)
    assert NO.barycentric_eval(e, pow(w, 3 % (1 << k), R)) == e[3 % (1 << k)]
