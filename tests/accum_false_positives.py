"""False positives of the one-word zero pre-test (fq_maybe_zero) that k_bucket_accumulate itself meets, found on the host.
TEST INFRASTRUCTURE ONLY (tests/test_field30_fused.py, tests/test_accum_false_positive_gpu.py).

k_affine96_to_table (srs_io.hip) stores fq_mul(fq_from_u32x12(w), fq_one()) for the words w of kzg_srs_load_affine, so the
level-0 table digits of a loaded SRS are what the g++ build of the same two calls returns, bit for bit
(tests/host/field30_fused_host.cpp: f30f_table_digits).  The second point of a bucket meets an accumulator that
xyzz30_acc_set has just written -- X = the first point's x, ZZ = fq_one_cold() -- so P = x_b one - x_a of xyzz30_acc_head
is known on the host too, and the pre-test looks at its low 30 bits only: a pair (a, b) fires when
low30(x_b one) - low30(x_a) is one of the seven residues k p mod 2^30.  One sorted lookup per residue over the rows
k G, k = 1 .. 65537, finds about a dozen unordered pairs that fire in both orders of arrival without being equal or
opposite (65537^2 / 2 pairs x 7 / 2^30); 20000 rows give none.
"""
import ctypes

import numpy as np

import bigint_twin as T

P = T.P
N_ROWS = 65537
LOW = (1 << 30) - 1
K_ACC_MAYBE_EQUAL = 4  # g1_30.hip.h

I32P = ctypes.POINTER(ctypes.c_int32)
U32P = ctypes.POINTER(ctypes.c_uint32)


def multiples_of_g(n):
    """[k G for k = 1 .. n] as affine integers: one Jacobian chain of mixed additions and one shared inversion"""
    jac, cur = [], (T.G1X, T.G1Y, 1)
    for _ in range(n):
        jac.append(cur)
        cur = T._jac_add_affine(cur[0], cur[1], cur[2], T.G1X, T.G1Y)
    prefix, run = [], 1
    for _, _, Z in jac:
        prefix.append(run)
        run = run * Z % P
    inv = pow(run, -1, P)
    out = [None] * n
    for i in range(n - 1, -1, -1):
        X, Y, Z = jac[i]
        zi = inv * prefix[i] % P
        inv = inv * Z % P
        zi2 = zi * zi % P
        out[i] = (X * zi2 % P, Y * zi2 % P * zi % P)
    return out


def affine_rows(points):
    """(n, 12) uint64 for kzg_srs_load_affine: x, y as blst_fp (Montgomery 2^384, canonical)"""
    raw = b"".join((c * T.FP_R % P).to_bytes(48, "little") for pt in points for c in pt)
    return np.frombuffer(raw, dtype=np.uint64).reshape(len(points), 12).copy()


def table_digits(lib, rows):
    """(n, 26) int32: the level-0 table digits (x, y) of the rows, from the g++ build of k_affine96_to_table's two calls"""
    words = np.ascontiguousarray(rows).view(np.uint32).reshape(-1, 12)
    out = np.empty((words.shape[0], 13), dtype=np.int32)
    lib.f30f_table_digits(words.ctypes.data_as(U32P), words.shape[0], out.ctypes.data_as(I32P))
    return out.reshape(rows.shape[0], 26)


def set_then_head(lib, digits, a, nega, b, negb):
    """(code, P is a multiple of p) of xyzz30_acc_head for row b on the accumulator xyzz30_acc_set leaves for row a"""
    zero = ctypes.c_int(0)
    code = lib.f30f_set_then_head(np.ascontiguousarray(digits[a]).ctypes.data_as(I32P), nega,
                                  np.ascontiguousarray(digits[b]).ctypes.data_as(I32P), negb, ctypes.byref(zero))
    return code, bool(zero.value)


def firing_pairs(lib, digits):
    """ordered pairs (a, b), a != b, for which the pre-test fires when b is added to the accumulator set from a: seven
    sorted lookups of low30(x_a) + (k p mod 2^30) among low30(x_b one)"""
    n = digits.shape[0]
    x = np.ascontiguousarray(digits[:, :13])
    lo_mul = np.empty(n, dtype=np.uint32)
    lo_x = np.empty(n, dtype=np.uint32)
    lib.f30f_low_bits(x.ctypes.data_as(I32P), n, lo_mul.ctypes.data_as(U32P), lo_x.ctypes.data_as(U32P))
    order = np.argsort(lo_mul, kind="stable")
    by_mul = lo_mul[order].astype(np.int64)
    found = set()
    for k in range(-3, 4):
        want = (lo_x.astype(np.int64) + ((k * P) & LOW)) & LOW
        lo, hi = np.searchsorted(by_mul, want, "left"), np.searchsorted(by_mul, want, "right")
        for a in np.nonzero(hi > lo)[0]:
            found.update((int(a), int(order[t])) for t in range(lo[a], hi[a]) if int(order[t]) != int(a))
    return found


def false_positive_pairs(lib, digits):
    """sorted unordered pairs (i, j), i < j, of different points that fire in BOTH orders of arrival; the host model of the
    head (set i, then head j, and the reverse, under every combination of the signs) must say code == kAccMaybeEqual with
    P != 0 for each of them"""
    ordered = firing_pairs(lib, digits)
    pairs = sorted((a, b) for a, b in ordered if a < b and (b, a) in ordered)
    for i, j in pairs:
        for a, b in ((i, j), (j, i)):
            for nega in (0, 1):
                for negb in (0, 1):
                    assert set_then_head(lib, digits, a, nega, b, negb) == (K_ACC_MAYBE_EQUAL, False), (a, nega, b, negb)
    return pairs
