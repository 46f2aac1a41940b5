"""CPU: tests/grand_product_oracle.py against itself, and the arithmetic of the grand-product kernels
(csrc/grand_product_kernels.hip) replayed on the host at the magnitudes their bound comments allow
(tests/host/gp_reach_host.cpp: a stand-alone program built with g++, nothing is loaded into this process)."""
import os
import random
import subprocess

import pytest

import fr_extremes as FE
import grand_product_oracle as GO

R = GO.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cols(t, n, seed):
    rnd = random.Random(seed)
    return [[rnd.randrange(1, R) for _ in range(n)] for _ in range(t)]


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 5, 64])
def test_checker_accepts_the_definition_and_nothing_else(n, t):
    nums, dens = _cols(t, n, 10 * n + t), _cols(t, n, 20 * n + t)
    z, last = GO.direct(nums, dens)
    assert z[0] == 1 and GO.check(nums, dens, z, last)
    assert not GO.check(nums, dens, z, (last + 1) % R)
    for at in sorted({0, n // 2, n - 1}):
        bad = list(z)
        bad[at] = (bad[at] + 1) % R
        assert not GO.check(nums, dens, bad, last), at
    if n > 1:  # a zero numerator: z is zero after it and so is last
        nums[0][n // 2] = 0
        z, last = GO.direct(nums, dens)
        assert all(v == 0 for v in z[n // 2 + 1:]) and last == 0 and GO.check(nums, dens, z, last)
    dens[t - 1][n - 1] = 0
    assert GO.first_zero(dens) == n - 1 and not GO.check(nums, dens, z, last)


def test_limb_conversion_round_trip():
    vals = [0, 1, R - 1, 0x1234567890ABCDEF << 100]
    limbs = GO.to_limbs(vals)
    assert limbs.shape == (4, 4) and GO.from_limbs(limbs) == vals
    assert [int(x) for x in limbs[1]] == [(GO.R256 >> (64 * i)) & (2**64 - 1) for i in range(4)]  # the image of one


@pytest.mark.parametrize("t", [1, 3, 5])
@pytest.mark.parametrize("k", [0, 1, 4])
def test_true_permutations_close_and_perturbed_wires_do_not(k, t):
    ks = GO.shifts(t)
    assert len({kj * p % R for kj in ks for p in GO.domain(k)}) == t << k  # the labels are distinct
    wires, sigmas = GO.true_permutation(k, t, ks, 100 * k + t)
    beta, gamma = 0x1111111111111111222222222222, 0x3333333333333333444444444444
    a, b = GO.perm_columns(wires, sigmas, ks, beta, gamma)
    z, last = GO.direct(a, b)
    assert last == 1 and GO.check(a, b, z, last)
    if (t << k) > 1:
        wires[t - 1][(1 << k) - 1] = (wires[t - 1][(1 << k) - 1] + 1) % R
        a, b = GO.perm_columns(wires, sigmas, ks, beta, gamma)
        moved = sigmas[t - 1][(1 << k) - 1] != ks[t - 1] * GO.domain(k)[-1] % R
        assert (GO.direct(a, b)[1] != 1) == moved  # a cell the permutation leaves alone may hold any value
    ident = GO.identity_sigmas(k, ks)
    a, b = GO.perm_columns(wires, ident, ks, beta, gamma)
    assert GO.direct(a, b) == ([1] * (1 << k), 1)


# ---- the kernels' arithmetic at its bounds -------------------------------------------------------------------------------------
RAW_BOUND = (1 << 30) + 8    # a sum of two carry-normalised values, or a normalised sum plus a product
NORM_BOUND = (1 << 29) + 4   # what fr30_norm, a load and a product leave in digits 0..7 (fr30.hip.h)
TOP_BOUND = 3 * 0x73EE       # a_j, b_j of the permutation form: below 2.51 r (grand_product_kernels.hip, "Bounds")
COLUMN_BOUND = 1 << 63       # a product's column fits the signed 64-bit accumulator
INV256 = pow(FE.R256, -1, R)


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gp") / "gp_reach")
    # -fwrapv: a digit sum that overflowed would wrap on the device, and so must it here
    subprocess.run(["g++", "-O2", "-fwrapv", "-o", exe, os.path.join(ROOT, "tests", "host", "gp_reach_host.cpp")], check=True)

    def run(form, t, tiles, head, lines):
        """head, lines: images.  Returns (report, exact-sum counts, bad index, last, z of the first K, z of the last K) -- images"""
        hexes = lambda row: " ".join("%064x" % v for v in row) + "\n"
        text = "%d %d %d %d\n" % (form, t, tiles, len(lines)) + (hexes(head) if head else "") + "".join(hexes(l) for l in lines)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
        K = len(lines)
        zs = [int(v, 16) for v in out[9:]]
        assert len(zs) == 2 * K
        return [int(v) for v in out[:4]], [int(v) for v in out[4:7]], int(out[7]), int(out[8], 16), zs[:K], zs[K:]

    return run


def _check_report(rep):
    assert rep[0] <= RAW_BOUND and rep[1] <= NORM_BOUND and rep[2] < TOP_BOUND and rep[3] < COLUMN_BOUND, rep


def _expected(tiles, A, B):
    """images of (last, z of the first K, z of the last K) for n = tiles x 1024 indices whose A_i, B_i repeat with period K"""
    K, n = len(A), tiles * 1024
    pre, acc = [], 1
    for a, b in zip(A, B):
        pre.append(acc)
        acc = acc * a % R * pow(b, R - 2, R) % R
    img = lambda v: v * FE.R256 % R
    head = pow(acc, n // K - 1, R)
    return img(pow(acc, n // K, R)), [img(p) for p in pre], [img(head * p % R) for p in pre]


@pytest.mark.parametrize("tiles", [1, 4096])
@pytest.mark.parametrize("t", [1, 16])
def test_replay_general_form_extremal_images(replay, t, tiles):
    """half values and digit-extremal images as factors, at both ends of the power-of-two bookkeeping (t = 1: no product
    before the scale, t = 16: fifteen) and of the carry scan (1 tile, 4096 tiles: 16 per lane)"""
    images = FE.half_values() + FE.digit_extremal() + [1, R - 1, FE.R256]
    K = 32
    lines = [[images[(5 * i + 3 * j) % len(images)] for j in range(t)] + [images[(7 * i + 11 * j + 1) % len(images)] for j in range(t)]
             for i in range(K)]
    rep, zsum, bad, last, first, tail = replay(0, t, tiles, None, lines)
    _check_report(rep)
    vals = [[v * INV256 % R for v in l] for l in lines]
    A, B = GO.products([[l[j] for l in vals] for j in range(t)]), GO.products([[l[t + j] for l in vals] for j in range(t)])
    assert bad == -1 and (last, first, tail) == _expected(tiles, A, B)
    assert first[0] == FE.R256  # z_0 is exactly the image of one


def _perm_lines(t, K, seed, mults):
    """(beta, gamma, ks, lines as values [w, f_0.., s_0..]) with extremal twiddles"""
    rnd = random.Random(seed)
    beta, gamma = rnd.randrange(1, R), rnd.randrange(R)
    ks = GO.shifts(t)
    lines = [[mults[i % len(mults)]] + [rnd.randrange(R) for _ in range(2 * t)] for i in range(K)]
    return beta, gamma, ks, lines


def _perm_run(replay, t, tiles, beta, gamma, ks, lines):
    img = lambda v: v % R * FE.R256 % R
    head = [img(beta), img(gamma)] + [img(beta * k) for k in ks]
    out = replay(1, t, tiles, head, [[img(v) for v in l] for l in lines])
    A = GO.products([[(l[1 + j] + beta * ks[j] % R * l[0] + gamma) % R for l in lines] for j in range(t)])
    B = GO.products([[(l[1 + j] + beta * l[1 + t + j] + gamma) % R for l in lines] for j in range(t)])
    return out, A, B


@pytest.mark.parametrize("tiles", [1, 4096])
@pytest.mark.parametrize("t", [1, 16])
def test_replay_permutation_form_extremal_twiddles(replay, t, tiles):
    beta, gamma, ks, lines = _perm_lines(t, 16, 77 + t, FE.extremal_multipliers())
    # f, sigma at image extremes as well: line 3 holds half values, line 5 digit-extremal images
    for j in range(2 * t):
        lines[3][1 + j] = FE.half_values()[j % 10] * INV256 % R
        lines[5][1 + j] = FE.digit_extremal()[j % 8] * INV256 % R
    (rep, zsum, bad, last, first, tail), A, B = _perm_run(replay, t, tiles, beta, gamma, ks, lines)
    _check_report(rep)
    assert bad == -1 and (last, first, tail) == _expected(tiles, A, B)


@pytest.mark.parametrize("multiple", [0, 1, 2])
def test_replay_zero_denominator_whose_sum_is_exactly_a_multiple_of_r(replay, multiple):
    """b = f + beta sigma + gamma = 0 with the integer sum of the two images and the lazy product at exactly 0, r and 2 r: outside
    what fr30_to_limbs canonicalises at 2 r, so the zero test must sit behind a reduction.  The product is the representative
    of -(f + gamma) within +-r/2, so the images of f and gamma choose the multiple: their sum 0.2 r -> 0, 1.1 r -> r, 1.85 r -> 2 r"""
    t, K, at, col = 3, 8, 5, 2
    beta, gamma, ks, lines = _perm_lines(t, K, 500 + multiple, [3, 5, 7])
    gamma_img, f_img = {0: (R // 10, R // 10), 1: (9 * R // 10, R // 5), 2: (9 * R // 10, 19 * R // 20)}[multiple]
    gamma, f = gamma_img * INV256 % R, f_img * INV256 % R
    lines[at][1 + col] = f
    lines[at][1 + t + col] = -(f + gamma) * pow(beta, R - 2, R) % R
    (rep, zsum, bad, last, first, tail), A, B = _perm_run(replay, t, 1, beta, gamma, ks, lines)
    _check_report(rep)
    assert B[at] == 0 and GO.first_zero([B]) == at
    assert bad == at
    assert zsum[multiple] == 1024 // K and sum(zsum) == 1024 // K, zsum  # every copy of the line, and no other sum
