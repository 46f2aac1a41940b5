"""Big-integer expectations for the powers-of-tau tests (tests/test_srs_ceremony.py, tests/test_srs_ceremony_gpu.py):
the scalar of every point after a contribution, the scalars of the two sums of the structure check, and the split of a
scalar for the endomorphism.  No group arithmetic: the tests turn a scalar v into [v]G1 with the C oracle."""
import bigint_twin as T

R = T.R
Z_ABS = 0xD201000000010000
LAMBDA = Z_ABS * Z_ABS - 1  # [LAMBDA](x, y) = (beta x, y) on G1; r = LAMBDA^2 + LAMBDA + 1
assert (LAMBDA * LAMBDA + LAMBDA + 1) == R


def scalar_of(be32):
    """32 big-endian bytes as kzg_srs_generate_g1 and kzg_srs_update read them: reduced mod r"""
    return int.from_bytes(bytes(be32), "big") % R


def setup_scalars(s, first, n):
    """the scalars of [s^(first + i)]G1, i < n (0^0 = 1)"""
    return [pow(s % R, first + i, R) for i in range(n)]


def updated_scalars(s, taus, first, n):
    """... after contributions tau_1, tau_2, ... in turn: point i becomes [(s tau_1 tau_2 ...)^(first + i)]G1"""
    t = s % R
    for tau in taus:
        t = t * (tau % R) % R
    return setup_scalars(t, first, n)


def lincomb_scalars(scalars, weights):
    """the scalars of A = sum_{i<n-1} rho_i SRS[i] and B = sum_{i<n-1} rho_i SRS[i+1] for SRS[i] = [scalars[i]]G1"""
    assert len(weights) == len(scalars) - 1
    a = sum(w * x for w, x in zip(weights, scalars[:-1])) % R
    b = sum(w * x for w, x in zip(weights, scalars[1:])) % R
    return a, b


def lambda_split(k):
    """(k1, k2) with k = k1 + k2 LAMBDA, k1 = k mod LAMBDA, k2 = k div LAMBDA: both below 2^128 for k < r"""
    assert 0 <= k < R
    return k % LAMBDA, k // LAMBDA
