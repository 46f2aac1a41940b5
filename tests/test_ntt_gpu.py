"""GPU: kzg_ntt / kzg_ntt_device (ntt_kernels.hip) element by element against the big-integer transforms of
tests/ntt_oracle.py, and at 2^20 / 2^22 against the C oracle's Horner evaluation at single domain points."""
import ctypes as C
import random

import numpy as np
import pytest

import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO

pytestmark = pytest.mark.gpu
R = NO.R
INPUTS = ["random", "zero", "r-1", "onehot0", "onehot_last", "constant"]


@pytest.fixture(scope="module")
def eng():
    e = K.Engine(0)  # no SRS: the transform needs none
    yield e
    e.close()


def _input(kind, n, seed):
    if kind == "random":
        rnd = random.Random(seed)
        return [rnd.randrange(R) for _ in range(n)]
    if kind == "zero":
        return [0] * n
    if kind == "r-1":
        return [R - 1] * n
    if kind == "onehot0":
        return [R - 2] + [0] * (n - 1)
    if kind == "onehot_last":
        return [0] * (n - 1) + [12345]
    return [R - 3] * n  # constant: its transform is one-hot


def _random_images(n, seed):
    """n random blst_fr images below r (top limb below r's): canonical, without a Python loop"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64, endpoint=False)
    c[:, 3] %= np.uint64(R >> 192)
    return c


def _ints(limbs):
    return K.limbs_to_scalars(limbs)


@pytest.mark.parametrize("k", list(range(0, 17)))
@pytest.mark.parametrize("kind", INPUTS)
def test_forward_and_inverse_elementwise(eng, k, kind):
    n = 1 << k
    v = _input(kind, n, 1000 + k)
    a = K.scalars_to_limbs(v)
    assert _ints(eng.ntt_limbs(a)) == NO.ntt(v), (k, kind, "forward")
    assert _ints(eng.intt_limbs(a)) == NO.intt(v), (k, kind, "inverse")


@pytest.mark.parametrize("k", [17, 18, 19, 20, 21, 22])  # radix-2^9 passes (9+8, 9+9), every three-pass plan
def test_large_round_trip_and_points(eng, oracle, k):
    n = 1 << k
    c = _random_images(n, k)
    e = eng.ntt_limbs(c)
    assert np.array_equal(eng.intt_limbs(e), c)
    w = NO.domain_root(k)
    rnd = random.Random(k)
    for j in [0, 1, n // 2, n - 1] + [rnd.randrange(n) for _ in range(64)]:
        want = oracle.poly_evaluate(c, oracle.fr_from_int(pow(w, j, R)))
        assert np.array_equal(e[j], want.reshape(4)), j


def test_magnitude_worst_case_2_22(eng):
    # What this reaches: the largest size, and every loaded value at the top of the canonical range (r - 1 as an integer),
    # so the product-free first stage of each pass holds 2 r.  What it does not reach: the bound of the later stages.  r - 1
    # is -1, and fr30_mul returns the centred residue, so from the second stage on every product is a small multiple of -1
    # (at most n in magnitude) and the sums stay at 2 r.  The inputs that add r / 2 per stage (6.5 r after eleven stages) are the chains of
    # tests/test_fr_extremes_gpu.py.
    n = 1 << 22
    a = K.scalars_to_limbs([R - 1]).repeat(n, axis=0)
    e = eng.ntt_limbs(a)  # sum_j (r - 1) w^(ij) = -n at i = 0, 0 elsewhere
    assert K.limbs_to_scalars(e[:1]) == [R - n]
    assert not e[1:].any()
    c = eng.intt_limbs(a)  # constant values r - 1: coefficient 0 is r - 1, the rest 0
    assert K.limbs_to_scalars(c[:1]) == [R - 1]
    assert not c[1:].any()


@pytest.mark.parametrize("k", [0, 5, 11, 12, 18, 19, 20])
def test_device_matches_host(eng, k):
    n = 1 << k
    rnd = random.Random(k)
    a = K.scalars_to_limbs([rnd.randrange(R) for _ in range(n)])
    lib = K.load_library()
    d_in, d_out = eng.dev_alloc(n * 32), eng.dev_alloc(n * 32)
    try:
        for inverse in (False, True):
            want = eng.intt_limbs(a) if inverse else eng.ntt_limbs(a)
            eng.dev_upload(d_in, a)
            eng.ntt_device(d_in, d_out, n, inverse)
            got = np.zeros_like(a)
            assert lib.kzg_dev_download(eng._h, got.ctypes.data, C.c_void_p(d_out), n * 32) == 0
            assert np.array_equal(got, want), (k, inverse)
            eng.ntt_device(d_in, d_in, n, inverse)  # in place
            assert lib.kzg_dev_download(eng._h, got.ctypes.data, C.c_void_p(d_in), n * 32) == 0
            assert np.array_equal(got, want), (k, inverse, "in place")
    finally:
        eng.dev_free(d_in)
        eng.dev_free(d_out)


def test_host_in_place_and_bad_sizes(eng):
    lib = K.load_library()
    rnd = random.Random(7)
    a = K.scalars_to_limbs([rnd.randrange(R) for _ in range(1 << 13)])
    want = eng.ntt_limbs(a)
    assert lib.kzg_ntt(eng._h, a.ctypes.data, a.shape[0], 0, a.ctypes.data) == 0
    assert np.array_equal(a, want)
    for n in (0, 3, 6, 1000, (1 << 22) + 1, 1 << 23):
        assert lib.kzg_ntt(eng._h, a.ctypes.data, n, 0, a.ctypes.data) == K.KZG_ERR_INVALID_ARG, n
        assert lib.kzg_ntt_device(eng._h, C.c_void_p(1), C.c_void_p(1), n, 0) == K.KZG_ERR_INVALID_ARG, n
