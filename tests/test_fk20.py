"""FK20 (kzg_cells_and_proofs_fk20) on the CPU: the algebra of tests/fk20_oracle.py against the stride-l synthetic
division of tests/cells_oracle.py with Fr standing in for G1, the GLV constants of csrc/fk20_kernels.hip against the
group law of oracle/bigint_twin.py, and the three new entry points in the library and the header."""
import os
import random
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)

import bigint_twin as T  # noqa: E402
import cells_oracle as CO  # noqa: E402
import fk20_oracle as F  # noqa: E402

R = F.R
Z = 0xD201000000010000  # |z| of BLS12-381
LAMBDA = Z * Z - 1
NEW_SYMBOLS = ("kzg_cells_and_proofs_fk20", "kzg_fk20_prepare", "kzg_g1_dft")


def _check(n, K, t, rng, trailing=0, srs_extra=0):
    vals = [rng.randrange(R) for _ in range(n)]
    if n:
        vals[-1] = vals[-1] or 1
    vals += [0] * trailing
    s = rng.randrange(1, R)
    n_eff = len(CO.trim(vals))
    l = 1 << t
    srs = [pow(s, i, R) for i in range(max(n_eff - l, 0) + srs_extra)]
    want = F.cell_proof_scalars(vals, K, t, s)
    assert F.fk20_proof_scalars(vals, K, t, srs, cached=True) == want, (n, K, t)
    assert F.fk20_proof_scalars(vals, K, t, srs, cached=False) == want, (n, K, t)
    if n_eff > l:
        assert F.toeplitz_h(vals, t, srs) == F.toeplitz_h_direct(vals, t, s)


@pytest.mark.parametrize("n,N,l", [(16, 32, 4), (13, 16, 2), (8, 8, 1), (64, 128, 8), (20, 32, 4), (5, 8, 4)])
def test_issue_shapes(n, N, l):
    rng = random.Random(n * 1000 + N + l)
    _check(n, N.bit_length() - 1, l.bit_length() - 1, rng)


@pytest.mark.parametrize("t", range(7))
def test_every_cell_size(t):
    """every l <= 64; n in {0, 1, l, l+1, 2l-1, non-powers of two, N} for N = l, 2l, 4l (and 8 for small l)"""
    rng = random.Random(77 + t)
    l = 1 << t
    for K in sorted({t, t + 1, t + 2, max(t, 3)}):
        N = 1 << K
        ns = {0, 1, l, l + 1, 2 * l - 1, N, N - 1, 3 * l + 1, (5 * N) // 7 + 1}
        for n in sorted(x for x in ns if 0 <= x <= N):
            _check(n, K, t, rng)


def test_trailing_zeros_and_larger_srs():
    rng = random.Random(5)
    _check(9, 5, 2, rng, trailing=7)            # n' = 9 inside n = 16
    _check(9, 5, 2, rng, srs_extra=40)          # the cached S_r reaches past n' - l
    _check(33, 6, 0, rng, srs_extra=100)


def test_glv_constants():
    """r = lambda^2 + lambda + 1, (beta x, y) = [lambda](x, y) for the beta whose digits fk20_kernels.hip holds"""
    assert LAMBDA * LAMBDA + LAMBDA + 1 == R
    src = open(os.path.join(ROOT, "kzg_poly_commit_exploration_amd", "csrc", "fk20_kernels.hip")).read()
    body = re.search(r"constexpr int32_t B\[13\] = \{([^}]*)\}", src).group(1)
    digits = [int(x.strip(), 16) if not x.strip().startswith("-") else -int(x.strip()[1:], 16) for x in body.split(",")]
    beta = sum(d << (30 * i) for i, d in enumerate(digits)) * pow(1 << 390, -1, T.P) % T.P
    assert pow(beta, 3, T.P) == 1 and beta != 1
    g = T.srs_g1(T.BENCH_SECRET_BE, 2)[1]
    for pt in (g, T.g1_mul(g, 12345)):
        assert T.g1_mul(pt, LAMBDA) == (pt[0] * beta % T.P, pt[1])
    # the host split w = k1 + k2 lambda keeps both halves below 2^128 for every w < r
    for w in (R - 1, LAMBDA, LAMBDA * LAMBDA, 1, 0):
        k2, k1 = divmod(w, LAMBDA)
        assert k1 < 1 << 128 and k2 < 1 << 128 and (k1 + k2 * LAMBDA) == w


def test_library_exports_fk20():
    import kzg_poly_commit_exploration_amd as K

    lib = K.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in K.ABI_SYMBOLS
    header = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
