"""CPU checks of tests/trapdoor_oracle.py: the trapdoor shortcuts against the oracle's MSM and quotient, the recoding model
by its defining identity, and the population builder by the segment geometry it promises."""
import random

import numpy as np
import pytest

import bigint_twin as T
import cells_oracle as CO
import ntt_oracle as NO
import open_points_oracle as OPO
import trapdoor_oracle as TO
import verify_cells_oracle as VO

R = TO.R


@pytest.mark.parametrize("s", [0, 1, R - 1, 2, 0x1234567890ABCDEF, R - 12345])
def test_commitment_and_proof_shortcuts_match_the_oracle(oracle, s):
    rnd = random.Random(s % 1000)
    n = 37
    srs = oracle.srs_g1(n, TO.secret_be(s))
    for vals in ([rnd.randrange(R) for _ in range(n)], [1] * n, [R - 1] * (n - 1) + [5]):
        c = oracle.fr_from_ints(vals)
        rc, want = oracle.commit_naive(c, srs)
        assert rc == 0
        assert TO.commitment(oracle, vals, s) == oracle.p1_compress(want)
        assert TO.commitment(oracle, vals, s) == oracle.p1_compress(oracle.commit_shortcut(c, TO.secret_be(s)))
        for z in (0, 1, R - 1, s, rnd.randrange(R)):  # z = s takes the derivative branch
            y = TO.poly_eval(vals, z)
            rc, want = oracle.generate_proof(c, oracle.fr_from_int(z), oracle.fr_from_int(y), srs)
            assert rc == 0
            assert TO.proof(oracle, vals, z, s) == oracle.p1_compress(want), (s, z)


@pytest.mark.parametrize("s", [0, 1, R - 1, 5, 0xDEADBEEF])
def test_multiproof_shortcut_matches_the_division_oracle(oracle, s):
    rnd = random.Random(s % 997)
    n = 29
    srs = oracle.srs_g1(n, TO.secret_be(s))
    vals = [rnd.randrange(R) for _ in range(n)]
    c = oracle.fr_from_ints(vals)
    for zs in ([0, 1, R - 1], [3, R - 3, 7, R - 7], list(range(1, 9)), [s, s + 1, rnd.randrange(R)]):
        ys = [TO.poly_eval(vals, z) for z in zs]
        rc, want = OPO.open_points(oracle, c, oracle.fr_from_ints(zs), oracle.fr_from_ints(ys), srs, threads=2)
        assert rc == 0
        assert TO.multiproof(oracle, vals, zs, s) == oracle.p1_compress(want), (s, zs)
        # and the quotient's value at s by the schoolbook division of the open-points oracle
        q, rem = OPO.poly_div_vanishing(vals, zs)
        assert TO.multiproof_scalar(vals, zs, s) == TO.poly_eval(q, s)


def test_fold_representative():
    assert TO.fold(0) == (0, False) and TO.fold(1) == (1, False) and TO.fold(R - 1) == (1, True)
    assert TO.fold(TO.HALF) == (TO.HALF, False)
    assert TO.fold(TO.HALF + 1) == (TO.HALF, True)  # (r+1)/2 = r - (r-1)/2
    assert TO.HALF < 1 << 254
    assert TO.near_fold_boundary(TO.HALF) and TO.near_fold_boundary(TO.HALF + 1) and not TO.near_fold_boundary(12345)


@pytest.mark.parametrize("c", list(range(8, 21)))
def test_window_recoding_identity_every_width(c):
    """sum_j d_j 2^(cj) = |k|, every digit in [-2^(c-1)+1, 2^(c-1)], for the edge family and random scalars"""
    W = TO.windows_of(c)
    rnd = random.Random(c)
    vals = TO.recoding_family(c) + [rnd.randrange(R) for _ in range(50)]
    lo, hi = -(1 << (c - 1)) + 1, 1 << (c - 1)
    for v in vals:
        mag, neg = TO.fold(v)
        d = TO.window_digits(mag, c, W)
        assert len(d) == W
        assert all(lo <= x <= hi for x in d), (c, v)
        assert sum(x << (c * j) for j, x in enumerate(d)) == mag, (c, v)
        assert (R - mag if neg else mag) == v % R
    # the edge cases the family is built for
    half = 1 << (c - 1)
    all_half = sum(half << (c * j) for j in range(W)) & ((1 << 254) - 1)
    if all_half <= TO.HALF:
        assert TO.window_digits(all_half, c, W)[:W - 1] == [half] * (W - 1)
    assert TO.window_digits(1, c, W) == [1] + [0] * (W - 1)
    assert TO.window_digits(half + 1, c, W)[:2] == [half + 1 - (1 << c), 1]  # a negative digit, the carry
    assert TO.count_refs([0, 1, R - 1, half, R - half], c) == 4


def test_msm_config_restates_the_chooser():
    # widths the suite's own tests rely on (test_gpu_parity.py: 2501 points -> 10 bits; degree 2^20 -> 17; 2^22 -> 19)
    assert TO.msm_config(2501)[:3] == (10, 26, 512)
    assert TO.msm_config((1 << 20) + 1)[:3] == (17, 15, 65536)
    assert TO.msm_config((1 << 22) + 1)[:3] == (19, 14, 262144)
    for c in (9, 11, 12, 14, 18):  # skipped by the chooser (top window of 1-3 bits), reachable when forced
        assert 254 - c * (TO.windows_of(c) - 1) < 4
        assert TO.msm_config(65537, forced_c=c)[0] == c
        assert all(TO.msm_config(n)[0] != c for n in (100, 1000, 2501, 65537, (1 << 20) + 1, (1 << 22) + 1))


def test_accumulation_geometry():
    assert TO.accumulate_lanes(15 * ((1 << 20) + 1)) == 131072
    assert TO.seg_len((1 << 20) + 1, 131072) == 9 and TO.seg_len(1 << 20, 131072) == 8
    assert TO.seg_len(65536, 131072) == 4 and TO.seg_len(65537, 131072) == 8  # kTinyRefs
    assert TO.accumulate_lanes(20 * 65537, 4096) == 4096 and TO.seg_len(65537, 4096) == 17
    assert TO.accumulate_lanes(100, 4096) == 256  # a multiple of the workgroup
    assert TO.tree_span_limit(65536) == TO.K_SERIAL_SPAN
    assert TO.finalize_group_size(4096) == 4 and TO.tree_span_limit(4096) == 64
    assert TO.pieces(0, 8, 8) == 1 and TO.pieces(0, 9, 8) == 2 and TO.pieces(7, 9, 8) == 2 and TO.pieces(7, 8, 8) == 1
    for L in (4, 8, 9, 17):
        for off in (0, 1, L - 1):
            for k in (1, 2, 16, 17, 65):
                lo, hi = TO.pieces_min_pop(k, off, L), TO.pieces_max_pop(k, off, L)
                assert TO.pieces(off, off + lo, L) == k and TO.pieces(off, off + hi, L) == k
                assert TO.pieces(off, off + hi + 1, L) == k + 1
                if lo > 1:
                    assert TO.pieces(off, off + lo - 1, L) == k - 1


@pytest.mark.parametrize("n_srs", [2501, 65537, (1 << 20) + 1])
@pytest.mark.parametrize("family", sorted(TO.FAMILIES))
def test_boundary_layouts_place_what_they_name(n_srs, family):
    job = TO.Job(n_srs, n_srs)
    M = n_srs
    pops, placed, L, S = TO.family_layout(family, job, M)
    assert sum(pops) == M and len(pops) == job.nb and pops[-1] > 0
    assert placed, family
    starts = np.concatenate([[0], np.cumsum(pops)])
    for label, (b, s, e, k) in placed.items():
        assert (starts[b], starts[b + 1]) == (s, e), label
        assert TO.pieces(s, e, L) == k
    vals = TO.values_from_pops(pops, random.Random(1))
    assert len(vals) == M
    got = [0] * job.nb
    for v in vals:
        mag, _ = TO.fold(v)
        d = TO.window_digits(mag, job.c, job.W)
        assert d[0] == mag and not any(d[1:])
        got[mag - 1] += 1
    assert got == pops
    if family == "tree_threshold":
        ks = {k for (_, _, _, k) in placed.values()}
        assert {S, S + 1} <= ks
    if family == "max_heavy" and n_srs > 65537:
        heavy = [k for (_, _, _, k) in placed.values()]
        assert all(k == S + 1 for k in heavy) and len(heavy) > 7000


def test_cube_root_of_unity():
    w = pow(7, (R - 1) // 3, R)
    assert w != 1 and pow(w, 3, R) == 1
    for k in (3, 4, 5):  # 2^k-th roots used by the scan tests
        u = pow(7, (R - 1) >> k, R)
        assert pow(u, 1 << k, R) == 1 and pow(u, 1 << (k - 1), R) != 1
    assert T.R == R


# ---- the data-availability references (tests/test_das_boundaries_gpu.py) ---------------------------------------------------
def _w(k):
    return NO.domain_root(k)


def _degenerate_secrets(K, t, L):
    """the secrets of the DAS boundary tests: 0, 1, r - 1, a cube root of unity, 2, a point of the domain (w_N^5: s^l = a_5
    when M > 5), an l-th root of unity (s^l = a_0 = 1), w_L (the FK20 convolution size) and one generic secret"""
    return {"0": 0, "1": 1, "r-1": R - 1, "omega3": pow(7, (R - 1) // 3, R), "2": 2, "w_N^5": pow(_w(K), 5, R),
            "w_l": _w(t), "w_L": _w(NO.log2_exact(L)), "generic": 0x1234567890ABCDEF}


@pytest.mark.parametrize("t", range(7))
def test_cell_proof_scalars_fast_against_fk20_oracle(t):
    """every cell, every degenerate secret, at shapes with one and several cells, n' at and below N"""
    import fk20_oracle as FO

    rnd = random.Random(100 + t)
    for K in sorted({t, t + 1, t + 3}):
        N, l = 1 << K, 1 << t
        for n in sorted({N, max(1, N - l + 1), min(N, l + 1)}):
            vals = [rnd.randrange(R) for _ in range(n)]
            L = FO.shape(n, t)[2]
            for name, s in _degenerate_secrets(K, t, L).items():
                want = FO.cell_proof_scalars(vals, K, t, s)
                got = TO.cell_proof_scalars_fast(vals, K, t, s)
                assert [got[j] for j in range(N >> t)] == want, (K, t, n, name)
            assert TO.cell_proof_scalars_fast(vals, K, t, 5, cells=[0])[0] == FO.cell_proof_scalars(vals, K, t, 5)[0]


def test_cell_proof_scalars_fast_takes_the_fallback():
    """s a point of cell 5 (s^l = a_5): the barycentric form would divide by zero there, the other cells keep it"""
    K, t = 8, 3
    s = pow(_w(K), 5 + 32 * 3, R)  # x_3 of cell 5
    assert pow(s, 8, R) == CO.cell_root(K, t, 5)
    vals = list(range(1, 200))
    got = TO.cell_proof_scalars_fast(vals, K, t, s)
    assert got[5] == CO.poly_eval(CO.stride_quotient(vals, 8, CO.cell_root(K, t, 5)), s)
    assert got[6] == CO.poly_eval(CO.stride_quotient(vals, 8, CO.cell_root(K, t, 6)), s)


@pytest.mark.parametrize("k", range(7))
def test_srs_dft_closed_form(k):
    m = 1 << k
    w = _w(k)
    for s in (0, 1, R - 1, 2, pow(7, (R - 1) // 3, R), 0xDEADBEEF, w, pow(w, m - 1, R), pow(w, 3 * (m > 3), R)):
        srs = [pow(s, i, R) for i in range(m)]
        want = NO.ntt(srs)
        assert TO.srs_dft_scalars(s, m) == want, (k, s)
    for j0 in range(m):  # s = w^-j0: m at j0, zero elsewhere
        got = TO.srs_dft_scalars(pow(w, (m - j0) % m, R), m)
        assert got[j0] == m % R and not any(got[:j0] + got[j0 + 1:])


def test_torsion_points_have_the_stated_orders():
    pts = TO.torsion_points()
    assert sorted(pts) == list(TO.TORSION_ORDERS)
    h = TO.H1
    for q in TO.TORSION_ORDERS:
        while h % q == 0:
            h //= q
    assert h == 1 and TO.H1 % 3 == 0 and TO.H1 % 9 != 0
    g = T.srs_g1(T.BENCH_SECRET_BE, 2)[1]
    for q, pt in list(pts.items()) + [(3, TO.ORDER3[0]), (3, TO.ORDER3[1])]:
        assert pt is not T.INF and T.g1_is_on_curve(pt)
        assert T.g1_mul(pt, q) is T.INF, q  # q prime: the order is q exactly
        assert not VO.g1_in_subgroup(pt) and not VO.g1_in_subgroup_by_order(pt), q
        bad = T.g1_add(g, pt)
        assert T.g1_is_on_curve(bad)
        assert not VO.g1_in_subgroup(bad) and not VO.g1_in_subgroup_by_order(bad), q
    assert VO.g1_in_subgroup(g)


@pytest.mark.parametrize("t", [0, 2, 3, 6])
def test_verification_algebra_under_degenerate_secrets(t):
    """LHS s^l = RHS for honest records, whatever the secret: s = 0, s^l = a_j, a root of unity, w_L"""
    import fk20_oracle as FO

    K = t + 3
    l, M = 1 << t, 8
    rnd = random.Random(t)
    polys = [[rnd.randrange(R) for _ in range(1 << K)], [R - 1] * (4 * l), [0] * (l - 1) + [1]]
    L = FO.shape(1 << K, t)[2]
    for name, s in _degenerate_secrets(K, t, L).items():
        coms, idx, ids, vals, prfs = [], [], [], [], []
        for b, p in enumerate(polys):
            coms.append(TO.poly_eval(p, s))
            cells = CO.cells(p, K, t)
            q = TO.cell_proof_scalars_fast(p, K, t, s)
            for j in range(M):
                idx.append(b)
                ids.append(j)
                vals.append(cells[j * l:(j + 1) * l])
                prfs.append(q[j])
        w = [rnd.randrange(R) for _ in ids]
        lhs, rhs = VO.scalar_sides(K, t, coms, idx, ids, vals, prfs, w, s)
        assert rhs == pow(s, l, R) * lhs % R, name
        v2 = [list(v) for v in vals]
        v2[3][0] = (v2[3][0] + 1) % R
        lhs2, rhs2 = VO.scalar_sides(K, t, coms, idx, ids, v2, prfs, w, s)
        assert rhs2 != pow(s, l, R) * lhs2 % R, name  # s = 0 too: the value enters through I(0)
