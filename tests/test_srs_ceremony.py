"""Powers-of-tau ceremonies, host side: kzg_g2_mul against the pairing twin, kzg_srs_verify_update on
links made with the oracle, the split oracle, the constants that srs_update_kernels.hip restates, and the compiler's metadata
of its kernels.  No GPU involved."""
import os
import random
import re

import numpy as np
import pytest

import bigint_twin as T
import kzg_poly_commit_exploration_amd as K
import pairing_twin as PT
import srs_ceremony_oracle as SO
from isa_cache import CSRC, kernel_meta, requires_hipcc

R, P = T.R, T.P
R_FP = 1 << 384


def _fp_mont_limbs(v):
    m = v * R_FP % P
    return [(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]


def _p2_limbs(pt, z=1):
    """affine G2 point of the twin (or INF) -> blst_p2 (Jacobian with Z = z), Montgomery limbs"""
    if pt is PT.INF:
        return np.zeros(36, dtype=np.uint64)
    (xa, xb), (ya, yb) = pt
    z2, z3 = z * z % P, z * z * z % P
    w = (_fp_mont_limbs(xa * z2) + _fp_mont_limbs(xb * z2) + _fp_mont_limbs(ya * z3) + _fp_mont_limbs(yb * z3)
         + _fp_mont_limbs(z) + _fp_mont_limbs(0))
    return np.array(w, dtype=np.uint64)


def _be(v):
    return int(v).to_bytes(32, "big")


@pytest.mark.parametrize("base", ["generator", "other"])
def test_g2_mul_against_the_pairing_twin(base):
    rnd = random.Random(13)
    q = PT.G2 if base == "generator" else PT.g2_mul(PT.G2, 0xC0FFEE)
    z = 1 if base == "generator" else 7  # a Jacobian input with Z != 1
    for k in (0, 1, R - 1, R + 5, rnd.randrange(R)):
        got = K.g2_mul(_p2_limbs(q, z), _be(k))
        assert np.array_equal(got, _p2_limbs(PT.g2_mul(q, k % R))), (base, k)
    # [s]G2 through either entry point
    assert np.array_equal(K.g2_mul(_p2_limbs(PT.G2), T.BENCH_SECRET_BE), K.srs_g2_at(T.BENCH_SECRET_BE, 1))


def test_g2_mul_refuses_a_point_off_the_twist():
    with pytest.raises(K.KzgError) as ei:
        K.g2_mul(_p2_limbs(((1, 2), (3, 4))), _be(5))
    assert ei.value.status == K.KZG_ERR_INVALID_ARG


def _g1(oracle, v):
    return K.G1Point(oracle.p1_mult(oracle.p1_generator(), v % R))


def test_verify_srs_update_links(oracle):
    rnd = random.Random(14)
    s, tau = rnd.randrange(1, R), rnd.randrange(2, R)
    before, after = _g1(oracle, s), _g1(oracle, s * tau)
    tau_g2 = K.g2_mul(_p2_limbs(PT.G2), _be(tau))
    assert K.verify_srs_update(before, after, tau_g2)
    # a wrong tau, the two points swapped, an `after` at infinity
    assert not K.verify_srs_update(before, after, K.g2_mul(_p2_limbs(PT.G2), _be((tau + 1) % R)))
    assert not K.verify_srs_update(after, before, tau_g2)
    inf = K.G1Point(np.zeros(18, dtype=np.uint64))
    assert not K.verify_srs_update(before, inf, tau_g2)
    assert not K.verify_srs_update(inf, inf, tau_g2)
    # tau = 1 links a point to itself; [tau]G2 at infinity is no link
    assert K.verify_srs_update(before, before, _p2_limbs(PT.G2))
    assert not K.verify_srs_update(before, before, np.zeros(36, dtype=np.uint64))
    # [tau]G2 off the twist: an error, as kzg_verify_proof answers it
    with pytest.raises(K.KzgError) as ei:
        K.verify_srs_update(before, after, _p2_limbs(((1, 2), (3, 4))))
    assert ei.value.status == K.KZG_ERR_INVALID_ARG


def test_verify_srs_update_refuses_tau_g2_outside_the_subgroup():
    """a point of the twist whose order is not r: found by walking x, then checked against [r]Q"""
    x = 1
    while True:
        x3b = PT.f2_add(PT.f2_mul(PT.f2_mul((x, 0), (x, 0)), (x, 0)), PT.B2)
        # a square root in Fp2 = Fp[u] / (u^2 + 1), p = 3 mod 4: y = x3b^((p^2 + 7) / 16) up to a fourth root of unity is
        # more than this needs; try the norm route instead
        a, b = x3b
        n = (a * a + b * b) % P
        if pow(n, (P - 1) // 2, P) == 1:
            sn = pow(n, (P + 1) // 4, P)
            for sgn in (sn, P - sn):
                half = (a + sgn) * pow(2, P - 2, P) % P
                if pow(half, (P - 1) // 2, P) == 1:
                    c = pow(half, (P + 1) // 4, P)
                    d = b * pow(2 * c, P - 2, P) % P
                    if PT.f2_mul((c, d), (c, d)) == x3b:
                        q = ((x, 0), (c, d))
                        assert PT.g2_is_on_curve(q)
                        acc = PT.INF  # [r]Q without the twin's reduction of the scalar
                        for bit in bin(R)[2:]:
                            acc = PT.g2_add(acc, acc)
                            if bit == "1":
                                acc = PT.g2_add(acc, q)
                        assert acc is not PT.INF
                        g = K.G1Point(np.array(T.g1_to_blst_p1_limbs(T.G1), dtype=np.uint64))
                        assert not K.verify_srs_update(g, g, _p2_limbs(q))
                        return
        x += 1


def test_split_oracle():
    assert SO.LAMBDA < 1 << 128 and SO.LAMBDA == 0xAC45A4010001A40200000000FFFFFFFF
    rnd = random.Random(15)
    for k in [0, 1, SO.LAMBDA - 1, SO.LAMBDA, SO.LAMBDA + 1, R - 1, SO.LAMBDA * SO.LAMBDA, SO.LAMBDA * SO.LAMBDA + SO.LAMBDA] \
            + [rnd.randrange(R) for _ in range(200)]:
        k1, k2 = SO.lambda_split(k)
        assert k1 + k2 * SO.LAMBDA == k and k1 < SO.LAMBDA and k2 <= SO.LAMBDA + 1 and max(k1, k2) < 1 << 128
    # the statement the ladder relies on: [k]P = [k1]P + [k2]phi(P), phi(x, y) = (beta x, y) = [LAMBDA](x, y)
    k1, k2 = SO.lambda_split(R - 2)
    g = T.G1
    phi = T.g1_mul(g, SO.LAMBDA)
    assert phi[1] == g[1] and pow(phi[0] * pow(g[0], P - 2, P) % P, 3, P) == 1
    assert T.g1_add(T.g1_mul(g, k1), T.g1_mul(phi, k2)) == T.g1_mul(g, R - 2)


def test_oracle_scalars():
    s, t1, t2 = 5, 7, 11
    assert SO.setup_scalars(s, 0, 3) == [1, 5, 25] and SO.setup_scalars(0, 0, 3) == [1, 0, 0]
    assert SO.updated_scalars(s, [t1], 1, 3) == [35, 35 ** 2, 35 ** 3]
    assert SO.updated_scalars(s, [t1, t2], 0, 3) == SO.updated_scalars(s, [t1 * t2], 0, 3) == [1, 385, 385 ** 2]
    assert SO.lincomb_scalars([1, 5, 25], [2, 3]) == (17, 85)
    assert SO.scalar_of(_be(R - 1)) == R - 1 and SO.scalar_of(b"\xff" * 32) == (2 ** 256 - 1) % R


def test_restated_constants_match():
    """srs_update_kernels.hip restates the GLV ladder of verify_kernels.hip and fk20_kernels.hip (the same digits of beta)
    and api.hip's lambda"""
    digits = []
    for name in ("fk20_kernels.hip", "verify_kernels.hip", "srs_update_kernels.hip"):
        body = re.search(r"constexpr int32_t B\[13\] = \{([^}]*)\}", open(os.path.join(CSRC, name)).read()).group(1)
        digits.append([int(x.strip(), 16) if not x.strip().startswith("-") else -int(x.strip()[1:], 16) for x in body.split(",")])
    assert digits[0] == digits[1] == digits[2]
    beta = sum(d << (30 * i) for i, d in enumerate(digits[2])) * pow(1 << 390, P - 2, P) % P
    assert T.g1_mul(T.G1, SO.LAMBDA) == (beta * T.G1[0] % P, T.G1[1])
    src = open(os.path.join(CSRC, "srs_update_kernels.hip")).read()
    hi, lo = re.search(r"kLambdaHi = (0x[0-9a-f]+)ULL, kLambdaLo = (0x[0-9a-f]+)ULL", src).groups()
    assert (int(hi, 16) << 64) | int(lo, 16) == SO.LAMBDA
    assert int(re.search(r"kBlsZAbs = (0x[0-9a-f]+)ULL", src).group(1), 16) == SO.Z_ABS


# ---- the compiler's metadata of the new kernels (as tests/test_verify_cells_isa.py) ------------------------------------------
@requires_hipcc
def test_srs_update_kernels_use_no_scratch():
    meta = kernel_meta("srs_update_kernels.hip")
    rec = {k: v for k, v in meta.items() if "k_srs_update" in k or "k_srs_check" in k}
    assert len(rec) == 2, sorted(meta)
    for name, m in rec.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
