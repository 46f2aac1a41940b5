"""Host-side checks of csrc/msm_recode.h (the scalar recoding of the MSM sort) against Python integers: the fold of a scalar
to sign and magnitude in both input forms, the 32-byte record the sort keeps between its two passes, and the digit loops --
the one that takes the window width at run time, the one compiled for a width, and the non-adjacent form.  CPU only: the
header is __host__ __device__ code, compiled here with g++."""
import ctypes
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
U8 = ctypes.c_uint32 * 8
CAP = 64
WIDTHS = list(range(8, 21))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("recode") / "librecode.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out,
                    os.path.join(ROOT, "tests", "host", "msm_recode_host.cpp")], check=True)
    return ctypes.CDLL(out)


def limbs(v):
    return [(v >> (32 * i)) & 0xffffffff for i in range(8)]


def value(words):
    return sum(int(w) << (32 * i) for i, w in enumerate(words))


def every_window(c, w):
    """the value below 2^254 whose every window of c bits holds w (the top window: what fits below bit 254)"""
    return sum(w << (c * j) for j in range((255 + c - 1) // c)) & ((1 << 254) - 1)


def edge_scalars():
    s = [0, 1, R - 1, (R - 1) // 2, (R + 1) // 2, ((1 << 254) - 1) % R]
    for c in WIDTHS:
        s += [every_window(c, 1 << (c - 1)) % R, every_window(c, (1 << (c - 1)) + 1) % R]
    return s


def scalars():
    rng = random.Random(2301)
    return edge_scalars() + [rng.randrange(R) for _ in range(300)]


def fold(lib, x, mont):
    k = U8()
    flip = lib.recode_host_fold(U8(*limbs((x << 256) % R if mont else x)), 1 if mont else 0, k)
    return flip, value(k)


def digits(fn, k, c):
    out = (ctypes.c_uint32 * (3 * CAP))()
    n = fn(U8(*limbs(k)), c, out, CAP)
    assert 0 <= n <= CAP
    return [(out[3 * i], out[3 * i + 1], out[3 * i + 2]) for i in range(n)]


def magnitudes(lib):
    """what the digit loops see: the folded scalars of both input forms, and the carry patterns as magnitudes themselves"""
    ks = set()
    for x in scalars():
        for mont in (True, False):
            ks.add(fold(lib, x, mont)[1])
    for c in WIDTHS:
        ks.add(every_window(c, 1 << (c - 1)))
        ks.add(every_window(c, (1 << (c - 1)) + 1))
        ks.add(every_window(c, (1 << c) - 1))
    ks.add((1 << 254) - 1)
    return sorted(ks)


def test_fold_gives_sign_and_magnitude_in_both_input_forms(lib):
    for x in scalars():
        seen = []
        for mont in (True, False):
            flip, k = fold(lib, x, mont)
            assert k < 1 << 254 and k <= R // 2 + (R >> 31) + 2
            assert ((-k if flip else k) - x) % R == 0, (x, mont)
            seen.append((flip, k))
        # the two sides of the fold: (r - 1) / 2 stays, (r + 1) / 2 is negated (up to the r / 2^31 the product leaves open)
        if x <= (R - 1) // 2 - (R >> 30):
            assert seen == [(0, x), (0, x)]
        if x >= (R + 1) // 2 + (R >> 30):
            assert seen == [(1, R - x), (1, R - x)]
    assert fold(lib, 0, True) == (0, 0) and fold(lib, 0, False) == (0, 0)
    assert fold(lib, R - 1, True) == (1, 1) and fold(lib, R - 1, False) == (1, 1)
    # canonical input is any 256-bit value: reduced as it is folded
    assert fold(lib, (1 << 254) - 1, False) == fold(lib, ((1 << 254) - 1) % R, False)


def test_record_keeps_the_magnitude_and_the_flag(lib):
    for k in magnitudes(lib):
        for flip in (0, 1):
            rec, back = U8(), U8()
            assert lib.recode_host_pack_roundtrip(U8(*limbs(k)), flip, rec, back) == flip
            assert value(back) == k
            assert value(rec) == k | (flip << 255)


@pytest.mark.parametrize("c", WIDTHS)
def test_window_digits_sum_to_the_magnitude_and_both_forms_agree(lib, c):
    W = (255 + c - 1) // c
    for k in magnitudes(lib):
        fixed = digits(lib.recode_host_windows_fixed, k, c)
        assert fixed == digits(lib.recode_host_windows_runtime, k, c), (c, hex(k))
        total, last = 0, -1
        for level, bucket, neg in fixed:
            assert last < level < W  # low window first, one digit per window at most
            last = level
            d = -(bucket + 1) if neg else bucket + 1
            assert -(1 << (c - 1)) + 1 <= d <= 1 << (c - 1) and d != 0
            total += d << (c * level)
        assert total == k, (c, hex(k))


@pytest.mark.parametrize("c", WIDTHS)
def test_a_carry_runs_through_every_window(lib, c):
    W = (255 + c - 1) // c
    # every window one above the half: each digit is negative and carries into the next, up to the top window
    d = digits(lib.recode_host_windows_fixed, every_window(c, (1 << (c - 1)) + 1), c)
    assert [neg for _, _, neg in d[:W - 1]] == [1] * (W - 1) and len(d) >= W - 1
    # every window exactly the half: the largest positive digit, no carry
    d = digits(lib.recode_host_windows_fixed, every_window(c, 1 << (c - 1)), c)
    assert all(neg == 0 for _, _, neg in d) and all(b == (1 << (c - 1)) - 1 for _, b, _ in d[:W - 1])


@pytest.mark.parametrize("c", WIDTHS + [21])
def test_naf_digits_sum_to_the_magnitude(lib, c):
    for k in magnitudes(lib):
        total, last = 0, -c
        for pos, bucket, neg in digits(lib.recode_host_naf, k, c):
            assert pos >= last + c and pos <= 254  # non-zero digits at least c bits apart
            last = pos
            d = 2 * bucket + 1
            assert d < 1 << (c - 1)
            total += (-d if neg else d) << pos
        assert total == k, (c, hex(k))


def test_widths_outside_the_compiled_range_are_refused(lib):
    out = (ctypes.c_uint32 * 3)()
    assert lib.recode_host_windows_fixed(U8(*limbs(1)), 7, out, 1) == -1
    assert lib.recode_host_windows_fixed(U8(*limbs(1)), 21, out, 1) == -1
