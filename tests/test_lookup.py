"""CPU: tests/lookup_oracle.py against itself, the arithmetic of the log-derivative kernels (csrc/lookup_kernels.hip) replayed
on the host at the magnitudes their bound comments allow (tests/host/lu_reach_host.cpp: a stand-alone program built with g++,
nothing is loaded into this process), and the NULL-context and argument errors of every new entry point, which need no GPU.

The replay's additive scans are fed twice: with real columns, where the results are compared with the definition, and with EVERY
term replaced by one sign-aligned extreme where it is accumulated (inputs cannot force 512 products of the same sign at 0.5 r).
The injected value, 0.506 r, is above what the unit's header allows any term (0.5002 r in the tile, 0.506 r in the carry kernel).

A denominator beta + f of the lookup form is the sum of two canonical images: it reaches exactly 0 (both zero) and exactly r,
and at most 2 r - 2, so "exactly 2 r" cannot occur in this design; the largest sum stands in for it."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import fr_extremes as FE
import kzg_poly_commit_exploration_amd as K
import lookup_oracle as LO

R = LO.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 512


def _cols(t, n, seed):
    rnd = random.Random(seed)
    return [[rnd.randrange(1, R) for _ in range(n)] for _ in range(t)]


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 5, 64])
def test_checker_accepts_the_definition_and_nothing_else(n, t):
    nums, dens = _cols(t, n, 10 * n + t), _cols(t, n, 20 * n + t)
    phi, last = LO.direct(nums, dens)
    assert phi[0] == 0 and LO.check(nums, dens, phi, last)
    assert not LO.check(nums, dens, phi, (last + 1) % R)
    for at in sorted({0, n // 2, n - 1}):
        bad = list(phi)
        bad[at] = (bad[at] + 1) % R
        assert not LO.check(nums, dens, bad, last), at
    ones = [[1] * n for _ in range(t)]
    assert LO.direct(None, dens) == LO.direct(ones, dens) and LO.check(None, dens, *LO.direct(ones, dens))
    nums[0][n // 2] = 0  # a zero numerator is legal
    assert LO.check(nums, dens, *LO.direct(nums, dens))
    dens[t - 1][n - 1] = 0
    assert LO.first_zero(dens) == n - 1 and not LO.check(nums, dens, phi, last)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("n", [1, 4, 33])
def test_valid_lookups_close_and_perturbed_ones_do_not(n, k):
    lookups, table, mult = LO.valid_lookup(n, k, 7 * n + k)
    counts, rows, missing = LO.multiplicities(table, lookups)
    assert missing is None and counts == mult and sum(counts) == k * n
    assert all(table[r] == v and table.index(v) == r for col, rs in zip(lookups, rows) for v, r in zip(col, rs))  # the LEAST row
    beta = 0x1111111111111111222222222222
    a, b = LO.lookup_columns(lookups, table, mult, beta)
    phi, last = LO.direct(a, b)
    assert last == 0 and LO.check(a, b, phi, 0)
    lookups[k - 1][n - 1] = (lookups[k - 1][n - 1] + 1) % R
    assert LO.multiplicities(table, lookups)[2] == n - 1 or lookups[k - 1][n - 1] in table
    a, b = LO.lookup_columns(lookups, table, mult, beta)
    assert LO.direct(a, b)[1] != 0
    assert LO.multiplicities([5, 6, 5, 5], [[5, 6, 5], [7, 5, 8]]) == ([3, 1, 0, 0], [[0, 1, 0], [None, 0, None]], 0)


# ---- the kernels' arithmetic at its bounds -------------------------------------------------------------------------------------
RAW_BOUND = (1 << 30) + 8    # a sum of two carry-normalised values, or a canonical value plus a product
NORM_BOUND = (1 << 29) + 4   # what fr30_norm, a load and a product leave in digits 0..7 (fr30.hip.h)
TOP_BOUND = 1 << 23          # |digit 8| of the additive scans (lookup_kernels.hip, "Bounds")
COLUMN_BOUND = 1 << 63       # a product's column fits the signed 64-bit accumulator
INV256 = pow(FE.R256, -1, R)
EXT = 506 * R // 1000        # the injected term, as an image


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lu") / "lu_reach")
    # -fwrapv: a digit sum that overflowed would wrap on the device, and so must it here
    subprocess.run(["g++", "-O2", "-fwrapv", "-o", exe, os.path.join(ROOT, "tests", "host", "lu_reach_host.cpp")], check=True)

    def run(form, t, tiles, lines, beta=None, inject=0):
        """lines: images.  Returns (report, exact-sum counts, bad row, last, phi of the first K, phi of the last K) -- images"""
        hexes = lambda row: " ".join("%064x" % v for v in row) + "\n"
        text = "%d %d %d %d %d\n" % (form, t, tiles, len(lines), inject) + hexes([EXT])
        text += (hexes([beta]) if form == 1 else "") + "".join(hexes(l) for l in lines)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
        k = len(lines)
        vals = [int(v, 16) for v in out[10:]]
        assert len(vals) == 2 * k
        return [int(v) for v in out[:5]], [int(v) for v in out[5:8]], int(out[8]), int(out[9], 16), vals[:k], vals[k:]

    def counts(cs):
        text = "2 1 1 %d 0\n%064x\n" % (len(cs), EXT) + "".join("%d\n" % c for c in cs)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
        return [int(v) for v in out[:5]], [int(v, 16) for v in out[5:]]

    run.counts = counts
    return run


def _check_report(rep):
    assert rep[0] <= RAW_BOUND and rep[1] <= NORM_BOUND and rep[2] < TOP_BOUND and rep[3] < COLUMN_BOUND and rep[4] == 0, rep


def _expected(tiles, nums, dens):
    """images of (last, phi of the first K, phi of the last K) for n = tiles x 512 rows whose columns repeat with period K"""
    k, n = len(dens[0]), tiles * T
    pre, period = LO.direct(nums, dens)
    img = lambda v: v % R * FE.R256 % R
    head = (n // k - 1) * period
    return img(n // k * period), [img(p) for p in pre], [img(head + p) for p in pre]


@pytest.mark.parametrize("tiles", [1, 8192])
@pytest.mark.parametrize("t", [1, 16])
def test_replay_general_form_extremal_images(replay, t, tiles):
    """half values and digit-extremal images in the fraction recurrence, at both ends of the power-of-two bookkeeping (t = 1: no
    step before the scale, t = 16: fifteen) and of the carry scans (1 tile, 8192 tiles: 32 per lane)"""
    images = FE.half_values() + FE.digit_extremal() + [1, R - 1, FE.R256]
    k = 32
    lines = [[images[(5 * i + 3 * j) % len(images)] for j in range(t)] + [images[(7 * i + 11 * j + 1) % len(images)] for j in range(t)]
             for i in range(k)]
    rep, zsum, bad, last, first, tail = replay(0, t, tiles, lines)
    _check_report(rep)
    vals = [[v * INV256 % R for v in l] for l in lines]
    nums, dens = [[l[j] for l in vals] for j in range(t)], [[l[t + j] for l in vals] for j in range(t)]
    assert bad == -1 and (last, first, tail) == _expected(tiles, nums, dens)
    assert first[0] == 0  # phi_0 is exactly the image of zero


@pytest.mark.parametrize("tiles", [1, 8192])
@pytest.mark.parametrize("t", [2, 16])
def test_replay_lookup_form(replay, t, tiles):
    rnd = random.Random(40 + t)
    k, kk = 16, t - 1
    images = FE.half_values() + FE.digit_extremal()
    beta = R - 5  # an image close to r: beta + f reaches nearly 2 r
    lines = [[images[(3 * i + j) % len(images)] if i % 2 else rnd.randrange(R) for j in range(kk)] + [rnd.randrange(R), rnd.randrange(1 << 26)]
             for i in range(k)]
    lines[3][0] = R - 1  # the largest sum of two canonical images, 2 r - 6 here
    rep, zsum, bad, last, first, tail = replay(1, t, tiles, lines, beta=beta)
    _check_report(rep)
    val = lambda v: v * INV256 % R
    lookups = [[val(l[j]) for l in lines] for j in range(kk)]
    a, b = LO.lookup_columns(lookups, [val(l[kk]) for l in lines], [val(l[kk + 1]) for l in lines], val(beta))
    assert bad == -1 and zsum == [0, 0, 0] and (last, first, tail) == _expected(tiles, a, b)


@pytest.mark.parametrize("inject", [1, 2])
@pytest.mark.parametrize("tiles", [1, 8192])
def test_replay_additive_scans_at_their_sign_aligned_extreme(replay, tiles, inject):
    """every w_i of the tile, every c_T W_T and every reduced lane sum of the carry kernel at +-0.506 r: the top digit stays below
    2^23, the columns of the products that take the sums stay inside 64 bits, and nothing outside (-r, 2 r) is stored"""
    lines = [[l[0], l[1]] for l in zip(*_cols(2, 8, 3))]
    rep, _, bad, _, _, _ = replay(0, 1, tiles, lines, inject=inject)
    _check_report(rep)
    assert bad == -1 and rep[2] > 255 * 0x73EE // 2  # the sums did reach the magnitude the bound is about


@pytest.mark.parametrize("case", ["zero", "r", "largest"])
def test_replay_lookup_denominator_whose_sum_is_a_multiple_of_r(replay, case):
    """beta + f as an integer sum of two canonical images at exactly 0 and exactly r -- a zero denominator, found behind the
    product with `scale` -- and at 2 r - 2, the largest there is, which is none"""
    t, k, at = 3, 8, 5
    rnd = random.Random(9)
    lines = [[rnd.randrange(1, R) for _ in range(t + 1)] for _ in range(k)]
    beta, f = {"zero": (0, 0), "r": (R // 3, R - R // 3), "largest": (R - 1, R - 1)}[case]
    lines[at][1] = f
    rep, zsum, bad, last, first, tail = replay(1, t, 1, lines, beta=beta)
    _check_report(rep)
    if case == "largest":
        assert bad == -1 and zsum == [0, 0, 0]
    else:
        assert bad == at and zsum == ([T // k, 0, 0] if case == "zero" else [0, T // k, 0])


def test_replay_counts_as_images(replay):
    cs = [0, 1, 2, 15 << 22, (1 << 26) - 1]
    rep, imgs = replay.counts(cs)
    _check_report(rep)
    assert imgs == [c * FE.R256 % R for c in cs]


# ---- arguments: no GPU is touched before they are refused ----------------------------------------------------------------------
def test_null_context_and_argument_errors_of_every_entry_point():
    lib = K.load_library()
    n, t = 8, 2
    a = LO.to_limbs(list(range(1, 2 * n + 1))).reshape(2, n, 4)
    out, last, p1, bad = np.zeros((n, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros(18, dtype=np.uint64), C.c_size_t(0)
    p = lambda x: x.ctypes.data
    b = C.byref(bad)
    inv = K.KZG_ERR_INVALID_ARG
    fake = C.c_void_p(0x1000)  # never dereferenced: the shape is refused first
    big = (1 << K.KZG_NTT_MAX_LOG) + 1
    assert K.KZG_LOGUP_MAX_COLUMNS == 16
    assert lib.kzg_logderivative_sum(None, p(a), p(a), n, t, n, p(out), p(last), b) == inv
    assert lib.kzg_logderivative_sum_device(None, p(a), p(a), n, t, n, p(out), p(last), b) == inv
    assert lib.kzg_lookup_sum(None, p(a), n, t, n, p(a), p(a), p(last), p(out), p(last), b) == inv
    assert lib.kzg_lookup_sum_device(None, p(a), n, t, n, p(a), p(a), p(last), p(out), p(last), b) == inv
    assert lib.kzg_lookup_commit(None, p(a), n, t, n, p(a), p(a), p(last), p(out), p(last), p(p1), b) == inv
    assert lib.kzg_batch_inverse(None, p(a), n, p(out), b) == inv
    assert lib.kzg_batch_inverse_device(None, p(a), n, p(out), b) == inv
    assert lib.kzg_lookup_multiplicities(None, p(a), n, p(a), n, t, n, p(out), None, b) == inv
    assert lib.kzg_lookup_multiplicities_device(None, p(a), n, p(a), n, t, n, p(out), None, b) == inv
    assert lib.kzg_lookup_multiplicities_cap(None, p(a), n, p(a), n, t, n, p(out), None, b, 4) == inv
    for n_, t_, s_ in ((0, t, n), (big, t, 1 << 23), (n, 0, n), (n, 17, n), (n, t, n - 1)):
        assert lib.kzg_logderivative_sum(fake, p(a), p(a), n_, t_, s_, p(out), p(last), b) == inv
        assert lib.kzg_logderivative_sum_device(fake, p(a), p(a), n_, t_, s_, p(out), p(last), b) == inv
    for n_, k_, s_ in ((0, t, n), (big, t, 1 << 23), (n, 0, n), (n, 16, n), (n, t, n - 1)):
        assert lib.kzg_lookup_sum(fake, p(a), n_, k_, s_, p(a), p(a), p(last), p(out), p(last), b) == inv
        assert lib.kzg_lookup_sum_device(fake, p(a), n_, k_, s_, p(a), p(a), p(last), p(out), p(last), b) == inv
        assert lib.kzg_lookup_commit(fake, p(a), n_, k_, s_, p(a), p(a), p(last), p(out), p(last), p(p1), b) == inv
        assert lib.kzg_lookup_multiplicities(fake, p(a), n, p(a), n_, k_, s_, p(out), None, b) == inv
        assert lib.kzg_lookup_multiplicities_device(fake, p(a), n, p(a), n_, k_, s_, p(out), None, b) == inv
        assert lib.kzg_lookup_multiplicities_cap(fake, p(a), n, p(a), n_, k_, s_, p(out), None, b, 4) == inv
    assert lib.kzg_lookup_commit(fake, p(a), 6, t, n, p(a), p(a), p(last), p(out), p(last), p(p1), b) == inv  # no power of two
    assert lib.kzg_lookup_commit(fake, p(a), n, t, n, p(a), p(a), p(last), p(out), p(last), None, b) == inv
    for n_ in (0, big):
        assert lib.kzg_batch_inverse(fake, p(a), n_, p(out), b) == inv
        assert lib.kzg_batch_inverse_device(fake, p(a), n_, p(out), b) == inv
        assert lib.kzg_lookup_multiplicities(fake, p(a), n_, p(a), n, t, n, p(out), None, b) == inv
        assert lib.kzg_lookup_multiplicities_device(fake, p(a), n_, p(a), n, t, n, p(out), None, b) == inv
    for cap in (2, K.KZG_NTT_MAX_LOG + 2):  # 2^log_capacity < n_table, and past the largest table
        assert lib.kzg_lookup_multiplicities_cap(fake, p(a), n, p(a), n, t, n, p(out), None, b, cap) == inv
    for null_at in (1, 2, 6):  # a NULL column or output
        args = [fake, p(a), p(a), n, t, n, p(out), p(last), b]
        args[null_at] = None
        if null_at != 1:  # nums == NULL is the form with numerators one
            assert lib.kzg_logderivative_sum(*args) == inv
    assert lib.kzg_batch_inverse(fake, None, n, p(out), b) == inv and lib.kzg_batch_inverse(fake, p(a), n, None, b) == inv
    assert lib.kzg_lookup_sum(fake, p(a), n, t, n, None, p(a), p(last), p(out), p(last), b) == inv
    assert lib.kzg_lookup_sum(fake, p(a), n, t, n, p(a), p(a), None, p(out), p(last), b) == inv
    assert lib.kzg_lookup_multiplicities(fake, p(a), n, p(a), n, t, n, None, None, b) == inv
