"""GPU: a device call writes its declared output and nothing else.

Every case lays ALL device operands of one call out in ONE guard-banded arena (tests/device_arena.py): the neighbours of an
output are the call's own inputs, every operand starts at an odd multiple of 32 bytes, strided operands use a stride of n + 5 and
their gaps are guard, and an output region is exactly as long as the header says the output is.  After the call the whole arena is
downloaded: the output equals the big-integer oracle's value (tests/*_oracle.py, never the library's own host form) and every
other byte -- inputs, guards, gaps -- is the byte that was uploaded.  tests/test_device_arena.py shows that a stray store fails
such a case and is named.

Sizes are the least that reach each path; the tile constants come from csrc/engine.h.  The calls that only read caller memory
(the _submit family) must leave the arena byte-identical, and their points are compared with the known-secret shortcut of
tests/trapdoor_oracle.py so that doing nothing does not pass.  Error returns leave everything but the output region intact.  The
host forms whose output length is not the obvious one get a numpy output larger than needed with the same fill.

Not covered: the library's internal workspaces (pq_ws, the slots' staging buffers, the circuit's scratch) are not reachable
through caller pointers, so a stray store inside them is not seen here; only the resident circuit columns that
kzg_circuit_column_device hands out are read back.  The _device forms take single-device contexts only."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import bigint_twin as BT
import device_arena as DA
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import lookup_oracle as LO
import ntt_oracle as NO
import open_combined_oracle as OC
import open_sets_oracle as SO
import perm_quotient_oracle as PQ
import test_circuit_open_gpu as TCO  # its memoised circuits, quotients and linearisations
import test_lookup_gpu as TL  # its memoised tables
import trapdoor_oracle as TO

pytestmark = pytest.mark.gpu
R = GO.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ENGINE_H = open(os.path.join(ROOT, "kzg_poly_commit_exploration_amd", "csrc", "engine.h")).read()


def _const(name):
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, _ENGINE_H).group(1))


GP_TILE, LU_TILE, PQ_TILE = _const("kGpTile"), _const("kLuTile"), _const("kPqTile")
S = BT.fr_from_be_bytes(BT.BENCH_SECRET_BE)
ALPHA, BETA, GAMMA = TCO.ALPHA, TCO.BETA, TCO.GAMMA
N_MIN = 4369  # the least length of the general sort and the accumulation kernel (tests/test_sort_single_recode_gpu.py)
NONE = C.c_size_t(-1).value
_CACHE = {}  # references computed once, shared and left unchanged


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _rand(n, seed, low=0):
    def make():
        rnd = random.Random(7919 * seed + n)
        return [rnd.randrange(low, R) for _ in range(n)]
    return _memo(("rand", n, seed, low), make)


def _cols(n, t, seed, low=0):
    return [_rand(n, 100 * seed + j, low) for j in range(t)]


def _lim(cols):
    """columns of equal length -> (t, n, 4): exactly the n values, the arena's stride leaves the gaps as guard"""
    return np.stack([GO.to_limbs(c) for c in cols])


@pytest.fixture(scope="module")
def eng():
    e = K.Engine(0)  # the transforms, products, sums and the permutation quotient's steps need no SRS
    yield e
    e.close()


def _raises(status, call):
    with pytest.raises(K.KzgError) as ei:
        call()
    assert ei.value.status == status, ei.value
    return ei.value


# ---- kzg_ntt_device ------------------------------------------------------------------------------------------------------------
def _ntt_case(n):
    def make():
        v = _rand(n, 1)
        return GO.to_limbs(v), GO.to_limbs(NO.ntt(v))
    return _memo(("ntt", n), make)


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("n", [1, 2, 1 << 10, 1 << 11, 1 << 12, 1 << 17])  # .., the last DFT size, one NTT tile, two passes, 9 + 8
def test_ntt_device(eng, n, inverse, in_place):
    coeffs, evals = _ntt_case(n)
    src, want = (evals, coeffs) if inverse else (coeffs, evals)
    with DA.Arena(eng, seed=n) as ar:
        d_in = ar.region(n, name="in", data=src)
        d_out = d_in if in_place else ar.region(n, name="out")
        ar.upload()
        eng.ntt_device(d_in.ptr, d_out.ptr, n, inverse)
        ar.check(outputs={d_out: want})  # out of place: the input is intact; in place: only that region changed


# ---- grand products ------------------------------------------------------------------------------------------------------------
GP_SIZES = [1, GP_TILE - 1, GP_TILE, GP_TILE + 1, 2 * GP_TILE + 1]


def _gp_arena(eng, a, b, n, t):
    """nums | z | dens: the output directly between the two inputs"""
    ar = DA.Arena(eng, seed=n + t)
    d_a = ar.region(n, t, n + 5, name="nums", data=_lim(a))
    d_z = ar.region(n, name="z")
    d_b = ar.region(n, t, n + 5, name="dens", data=_lim(b))
    ar.upload()
    return ar, d_a, d_z, d_b


@pytest.mark.parametrize("t", [1, 3, K.KZG_GP_MAX_COLUMNS])
@pytest.mark.parametrize("n", GP_SIZES)
def test_grand_product_device(eng, n, t):
    nums, dens = _cols(n, t, 2), _cols(n, t, 3, low=1)
    z, last = _memo(("gp", n, t), lambda: GO.direct(nums, dens))
    ar, d_a, d_z, d_b = _gp_arena(eng, nums, dens, n, t)
    with ar:
        got_last = eng.grand_product_device(d_a.ptr, d_b.ptr, n, t, d_z.ptr, stride=n + 5)
        assert GO.from_limbs(got_last) == [last]
        ar.check(outputs={d_z: GO.to_limbs(z)})


@pytest.mark.parametrize("t", [1, 3, K.KZG_GP_MAX_COLUMNS])
@pytest.mark.parametrize("n", [1, GP_TILE, 2 * GP_TILE])  # the permutation form takes powers of two
def test_permutation_product_device(eng, n, t):
    ks = GO.shifts(t)
    wires, sigmas = _cols(n, t, 4), _cols(n, t, 5)

    def make():
        a, b = GO.perm_columns(wires, sigmas, ks, BETA, GAMMA)
        assert GO.first_zero(b) is None
        return GO.direct(a, b)
    z, last = _memo(("perm", n, t), make)
    ar, d_w, d_z, d_s = _gp_arena(eng, wires, sigmas, n, t)
    with ar:
        got_last = eng.permutation_product_device(d_w.ptr, d_s.ptr, n, t, [K.Scalar(k) for k in ks], K.Scalar(BETA), K.Scalar(GAMMA),
                                                  d_z.ptr, stride=n + 5)
        assert GO.from_limbs(got_last) == [last]
        ar.check(outputs={d_z: GO.to_limbs(z)})


# ---- running sums and the batch inverse ----------------------------------------------------------------------------------------
LU_SIZES = [1, LU_TILE - 1, LU_TILE, LU_TILE + 1, 2 * LU_TILE + 1]


def _running_sum(nums, dens):
    """lookup_oracle.direct with ntt_oracle.batch_inverse for its n t inversions, and the oracle's own inversion-free check of the
    result, which has one solution.  direct itself raises to the power r - 2 once per fraction: 2.5 s at n = 1025, t = 16, for
    each of the cases of that size"""
    n, t = len(dens[0]), len(dens)
    inv = NO.batch_inverse([b[i] for i in range(n) for b in dens])
    phi, acc = [], 0
    for i in range(n):
        phi.append(acc)
        for j in range(t):
            acc = (acc + (1 if nums is None else nums[j][i]) * inv[i * t + j]) % R
    assert LO.check(nums, dens, phi, acc)
    return phi, acc


@pytest.mark.parametrize("with_nums", [True, False], ids=["nums", "nums_null"])
@pytest.mark.parametrize("t", [1, K.KZG_LOGUP_MAX_COLUMNS])
@pytest.mark.parametrize("n", LU_SIZES)
def test_logderivative_sum_device(eng, n, t, with_nums):
    nums, dens = (_cols(n, t, 6) if with_nums else None), _cols(n, t, 7, low=1)
    phi, last = _memo(("lds", n, t, with_nums), lambda: _running_sum(nums, dens))
    with DA.Arena(eng, seed=n + t) as ar:
        d_a = ar.region(n, t, n + 5, name="nums", data=_lim(nums)) if with_nums else None
        d_phi = ar.region(n, name="phi")
        d_b = ar.region(n, t, n + 5, name="dens", data=_lim(dens))
        ar.upload()
        got_last = eng.logderivative_sum_device(d_a.ptr if with_nums else None, d_b.ptr, n, t, d_phi.ptr, stride=n + 5)
        assert LO.from_limbs(got_last) == [last]
        ar.check(outputs={d_phi: LO.to_limbs(phi)})


@pytest.mark.parametrize("k", [1, K.KZG_LOGUP_MAX_COLUMNS - 1])
@pytest.mark.parametrize("n", LU_SIZES)
def test_lookup_sum_device(eng, n, k):
    lookups, table, mult = _cols(n, k, 8), _rand(n, 9), [v % 7 for v in _rand(n, 10)]  # any columns: last is what it is

    def make():
        a, b = LO.lookup_columns(lookups, table, mult, BETA)
        assert LO.first_zero(b) is None
        return _running_sum(a, b)
    phi, last = _memo(("lus", n, k), make)
    with DA.Arena(eng, seed=n + k) as ar:
        d_f = ar.region(n, k, n + 5, name="lookups", data=_lim(lookups))
        d_phi = ar.region(n, name="phi")
        d_t = ar.region(n, name="table", data=LO.to_limbs(table))
        d_m = ar.region(n, name="mult", data=LO.to_limbs(mult))
        ar.upload()
        got_last = eng.lookup_sum_device(d_f.ptr, n, k, d_t.ptr, d_m.ptr, K.Scalar(BETA), d_phi.ptr, stride=n + 5)
        assert LO.from_limbs(got_last) == [last]
        ar.check(outputs={d_phi: LO.to_limbs(phi)})


@pytest.mark.parametrize("n", LU_SIZES)
def test_batch_inverse_device(eng, n):
    vals = _rand(n, 11, low=1)
    with DA.Arena(eng, seed=n) as ar:
        d_out = ar.region(n, name="out")
        d_v = ar.region(n, name="vals", data=LO.to_limbs(vals))
        ar.upload()
        eng.batch_inverse_device(d_v.ptr, n, d_out.ptr)
        inv = NO.batch_inverse(vals)
        assert all(v * w % R == 1 for v, w in zip(vals, inv))
        ar.check(outputs={d_out: LO.to_limbs(inv)})


# ---- multiplicities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_rows", [True, False], ids=["rows", "rows_null"])
@pytest.mark.parametrize("n,k", [(1, 1), (257, 3)])
@pytest.mark.parametrize("n_table", [1, 255, 256, 257])
def test_lookup_multiplicities_device(eng, n_table, n, k, with_rows):
    table = TL._table(n_table)
    lookups = TL._draw(table, n, k, n_table + n)
    counts, rows, missing = LO.multiplicities(table, lookups)
    assert missing is None
    with DA.Arena(eng, seed=n_table + n) as ar:
        d_t = ar.region(n_table, name="table", data=LO.to_limbs(table))
        d_m = ar.region(n_table, name="mult")
        d_f = ar.region(n, k, n + 5, name="lookups", data=_lim(lookups))
        d_r = ar.region(n, k, name="rows", row_bytes=4) if with_rows else None  # k n 32-bit words: the end falls mid-row
        ar.region(1, name="after_rows", data=LO.to_limbs([1]))  # what follows the words is an input of the arena
        ar.upload()
        eng.lookup_multiplicities_device(d_t.ptr, n_table, d_f.ptr, n, k, d_m.ptr, d_r.ptr if with_rows else None, stride=n + 5)
        outputs = {d_m: LO.to_limbs(counts)}
        if with_rows:
            outputs[d_r] = np.array(rows, dtype=np.uint32)
        ar.check(outputs=outputs)


# ---- the coset extension -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["values", "coeffs_3", "coeffs_N-1"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("N", [4, 256, 2048, 4096])  # the DFT below 2^11, one NTT tile, two passes
def test_coset_extend_device(eng, N, batch, kind):
    log_N = NO.log2_exact(N)
    length = {"values": max(1, N // 4), "coeffs_3": 3, "coeffs_N-1": N - 1}[kind]
    form = K.KZG_EXTEND_VALUES if kind == "values" else K.KZG_EXTEND_COEFFS

    def make(j):
        col = _rand(length, 20 + j)
        return col, PQ.coset_extend(NO.intt(col) if kind == "values" else col, log_N)
    cases = [_memo(("ext", N, kind, j), lambda j=j: make(j)) for j in range(batch)]
    with DA.Arena(eng, seed=N + batch) as ar:
        d_in = ar.region(length, batch, length + 5, name="in", data=_lim([c[0] for c in cases]))
        d_out = ar.region(N, batch, name="out")  # batch * N packed
        ar.upload()
        eng.coset_extend_device(d_in.ptr, length, batch, log_N, d_out.ptr, form=form, stride=length + 5)
        ar.check(outputs={d_out: _lim([c[1] for c in cases])})


# ---- the constraints on the coset ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_gate", [True, False], ids=["gate", "gate_null"])
@pytest.mark.parametrize("N,t", [(2, 1), (PQ_TILE, 1), (2 * PQ_TILE, 1), (8, 7), (PQ_TILE, 7), (2 * PQ_TILE, 7)])
def test_permutation_constraints_coset_device(eng, N, t, with_gate):
    """N is a power of two: below, at and at twice the tile of k_pq_constraints.  t = 7 needs rot = 8, so its least N is 8"""
    rot = 2 if t == 1 else 8
    n = N // rot
    ks = GO.shifts(t)
    wires, sigmas, z, gate = _cols(N, t, 30), _cols(N, t, 31), _rand(N, 32), (_rand(N, 33) if with_gate else None)
    want = _memo(("pqc", N, t, with_gate), lambda: PQ.constraints_on_coset(wires, sigmas, z, n, ks, ALPHA, BETA, GAMMA, gate))
    with DA.Arena(eng, seed=N + t) as ar:
        d_w = ar.region(N, t, N + 5, name="wires", data=_lim(wires))
        d_out = ar.region(N, name="out")
        d_s = ar.region(N, t, N + 5, name="sigmas", data=_lim(sigmas))
        d_z = ar.region(N, name="z", data=GO.to_limbs(z))
        d_g = ar.region(N, name="gate", data=GO.to_limbs(gate)) if with_gate else None
        ar.upload()
        eng.permutation_constraints_coset_device(d_w.ptr, d_s.ptr, d_z.ptr, n, rot, t, [K.Scalar(k) for k in ks], K.Scalar(ALPHA),
                                                 K.Scalar(BETA), K.Scalar(GAMMA), d_out.ptr, d_gate=d_g.ptr if with_gate else None,
                                                 stride=N + 5)
        ar.check(outputs={d_out: GO.to_limbs(want)})


# ---- the vanishing quotient ----------------------------------------------------------------------------------------------------
def _vq_case(n, e):
    """(T of degree N - n - 1 exactly, the values of T (X^n - 1) on the coset, those values over Z_H)"""
    def make():
        N = n * e
        log_N = NO.log2_exact(N)
        T = _rand(N - n, 40)[:-1] + [1 + _rand(1, 41)[0] % (R - 1)]
        num = [((T[k - n] if k >= n else 0) - (T[k] if k < N - n else 0)) % R for k in range(N)]
        return T, PQ.coset_extend(num, log_N), PQ.coset_extend(T + [0] * n, log_N)
    return _memo(("vq", n, e), make)


@pytest.mark.parametrize("already_divided", [False, True], ids=["num", "divided"])
@pytest.mark.parametrize("n,e", [(1, 2), (2, 8), (512, 4), (1024, 2)])
def test_vanishing_quotient_device(eng, n, e, already_divided):
    N = n * e
    T, num, divided = _vq_case(n, e)
    with DA.Arena(eng, seed=N) as ar:
        d_in = ar.region(N, name="num", data=GO.to_limbs(divided if already_divided else num))
        d_out = ar.region(N - n, name="T")  # exactly N - n rows: the trailing guard starts where N rows would have slack
        ar.upload()
        eng.vanishing_quotient_device(d_in.ptr, N, n, d_out.ptr, already_divided=already_divided)
        ar.check(outputs={d_out: GO.to_limbs(T)})


# ---- a circuit: quotient, then the opening, on one arena; the resident key is left as it was ---------------------------------
def _resident(e, circ, t):
    """every column kzg_circuit_column_device hands out, in every form it accepts: {(which, form): bytes}"""
    which = [K.KZG_CIRCUIT_COL_QLIN + j for j in range(t)] + [K.KZG_CIRCUIT_COL_QM, K.KZG_CIRCUIT_COL_QC] + \
            [K.KZG_CIRCUIT_COL_SIGMA + j for j in range(t)]
    keys = [(w, f) for w in which for f in (K.KZG_CIRCUIT_VALUES, K.KZG_CIRCUIT_COEFFS, K.KZG_CIRCUIT_COSET)]
    keys.append((K.KZG_CIRCUIT_COL_L0, K.KZG_CIRCUIT_COSET))
    out = {}
    for key in keys:
        p, ln = circ.column_device(*key)
        got = np.zeros((ln, 4), dtype=np.uint64)
        assert e._lib.kzg_dev_download(e._h, got.ctypes.data, C.c_void_p(p), ln * 32) == 0
        out[key] = got
    return out


@pytest.mark.parametrize("with_pi", [True, False], ids=["pi", "pi_null"])
@pytest.mark.parametrize("n,t,log_ext", [(1, 3, 2), (256, 3, 2), (2048, 3, 2), (4096, 2, 2), (64, 7, 3)])
def test_circuit_quotient_then_open_device(engines, oracle, n, t, log_ext, with_pi):
    N = n << log_ext
    e = engines.bench_srs(TCO.SRS)
    c, z, T, coefs = TCO._case(n, t, with_pi)
    r, evals, stack = TCO._lin(n, t, log_ext, with_pi)
    want_t = TCO._t_limbs(T, n, log_ext)
    circ = TCO._create(e, c, log_ext)
    try:
        before = _resident(e, circ, t)
        with DA.Arena(e, seed=n + t) as ar:
            d_w = ar.region(n, t, n + 5, name="wires", data=_lim(c.wires))
            d_t = ar.region(N - n, name="T")
            d_z = ar.region(n, name="z", data=GO.to_limbs(z))
            d_pi = ar.region(n, name="pi", data=GO.to_limbs(c.pi)) if with_pi else None
            ar.upload()
            pi = d_pi.ptr if with_pi else None
            circ.quotient_device(d_w.ptr, d_z.ptr, *TCO._ch()[:3], d_t.ptr, d_public_inputs=pi, stride=n + 5)
            got_evals, proof = circ.open_device(d_w.ptr, d_z.ptr, d_t.ptr, *TCO._ch(), d_public_inputs=pi, stride=n + 5)
            assert TCO._values(got_evals) == evals
            assert proof.compress() == TO.g1_scalar(oracle, SO.proof_scalar(stack[0], stack[1], stack[2], TCO.V, S))
            ar.check(outputs={d_t: want_t})
            after = _resident(e, circ, t)
            assert before.keys() == after.keys()
            for key in before:
                assert np.array_equal(before[key], after[key]), key  # (which, form) of the resident column that changed
            circ.quotient_device(d_w.ptr, d_z.ptr, *TCO._ch()[:3], d_t.ptr, d_public_inputs=pi, stride=n + 5)  # the key still serves
            ar.check(outputs={d_t: want_t})
    finally:
        circ.close()


# ---- calls that only read caller memory ----------------------------------------------------------------------------------------
def _poly(n, j=0):
    return _rand(n, 50 + j)


def _read_only(e, n, cols=1, stride=None, seed=0, values=None):
    """one region holding `cols` polynomials of n values; the caller uploads, runs its job and calls check_untouched()"""
    ar = DA.Arena(e, seed=n + cols + seed)
    polys = [_poly(n, j) for j in range(cols)] if values is None else values
    d = ar.region(n, cols, stride, name="polys", data=_lim(polys))
    ar.upload()
    return ar, d, polys


@pytest.mark.parametrize("n", [4096, N_MIN])
def test_commit_submit_reads_only(engines, oracle, n):
    e = engines.bench_srs(N_MIN)
    ar, d, (vals,) = _read_only(e, n)
    with ar:
        e.commit_submit(0, d.ptr, n)
        assert e.wait(0).compress() == _memo(("commit", n), lambda: TO.commitment(oracle, vals, S))
        ar.check_untouched()


@pytest.mark.parametrize("n", [2049, 4096, N_MIN])
def test_open_submit_reads_only(engines, oracle, n):
    e = engines.bench_srs(N_MIN)
    ar, d, (vals,) = _read_only(e, n)
    z = _rand(1, 60)[0]
    y = TO.poly_eval(vals, z)
    with ar:
        e.open_submit(0, d.ptr, n, K.Scalar(z), K.Scalar(y))
        assert e.wait(0).compress() == TO.proof(oracle, vals, z, S, y)
        ar.check_untouched()


@pytest.mark.parametrize("n", [2049, 4096, N_MIN])  # 2049: one tile and one value of the opening's scan, one per polynomial
def test_batch_submits_read_only(engines, oracle, n):
    """kzg_commit_batch_submit and kzg_open_batch_submit: batch 2, stride n + 37"""
    e = engines.bench_srs(N_MIN)
    stride = n + 37
    ar, d, polys = _read_only(e, n, cols=2, stride=stride)
    zs = _rand(2, 61)
    ys = [TO.poly_eval(p, z) for p, z in zip(polys, zs)]
    before = e.max_batch()
    with ar:
        try:
            assert e.set_max_batch(2) == 2
            e.commit_batch_submit(0, d.ptr, n, 2, stride)
            got = e.wait_batch(0, 2)
            assert [g.compress() for g in got] == [TO.commitment(oracle, p, S) for p in polys]
            ar.check_untouched()
            zl, yl = GO.to_limbs(zs), GO.to_limbs(ys)
            assert e._lib.kzg_open_batch_submit(e._h, 0, C.c_void_p(d.ptr), n, 2, stride, zl.ctypes.data, yl.ctypes.data) == K.KZG_OK
            out, st = np.zeros((2, 18), dtype=np.uint64), np.zeros(2, dtype=np.int32)
            assert e._lib.kzg_wait_open_batch(e._h, 0, out.ctypes.data, st.ctypes.data, 2) == K.KZG_OK
            assert st.tolist() == [K.KZG_OK, K.KZG_OK]
            assert [K.G1Point(p).compress() for p in out] == [TO.proof(oracle, p, z, S, y) for p, z, y in zip(polys, zs, ys)]
            ar.check_untouched()
        finally:
            e.set_max_batch(before)


@pytest.mark.parametrize("n", [2049, 4096, N_MIN])
def test_open_points_submit_reads_only(engines, oracle, n):
    e = engines.bench_srs(N_MIN)
    ar, d, (vals,) = _read_only(e, n)
    zs = _rand(3, 62)
    ys = [TO.poly_eval(vals, z) for z in zs]
    with ar:
        e.open_points_submit(0, d.ptr, n, [K.Scalar(z) for z in zs], [K.Scalar(y) for y in ys])
        assert e.wait(0).compress() == TO.multiproof(oracle, vals, zs, S, ys)
        ar.check_untouched()


@pytest.mark.parametrize("n", [2049, 4096, N_MIN])
def test_open_combined_submit_reads_only(engines, oracle, n):
    e = engines.bench_srs(N_MIN)
    t = 3
    ar, d, polys = _read_only(e, n, cols=t, stride=n + 5)
    z, gamma = _rand(2, 63)
    with ar:
        e.open_combined_submit(0, d.ptr, n, t, K.Scalar(z), K.Scalar(gamma), stride=n + 5)
        ys, proof = e.wait_combined(0, t)
        assert [y.v for y in ys] == OC.values(polys, z)
        assert proof.compress() == TO.g1_scalar(oracle, OC.proof_scalar(OC.combine(polys, gamma), z, S))
        ar.check_untouched()


@pytest.mark.parametrize("n", [2049, 4096, N_MIN])
def test_open_sets_submit_reads_only(engines, oracle, n):
    e = engines.bench_srs(N_MIN)
    t, set_of = 4, [0, 1, 0, 1]
    a, b, c, gamma = _rand(4, 64)
    sets = [[a], [b, c]]
    ar, d, polys = _read_only(e, n, cols=t, stride=n + 5)
    ksets = [[K.Scalar(x) for x in s] for s in sets]
    with ar:
        e.open_sets_submit(0, d.ptr, n, t, set_of, ksets, K.Scalar(gamma), stride=n + 5)
        ys, proof = e.wait_sets(0, set_of, ksets)
        assert [[y.v for y in row] for row in ys] == SO.values(polys, set_of, sets)
        assert proof.compress() == TO.g1_scalar(oracle, SO.proof_scalar(polys, set_of, sets, gamma, S))
        ar.check_untouched()


def _evals_case(n):
    def make():
        e = _rand(n, 70)
        return e, NO.intt(e)
    return _memo(("evals", n), make)


@pytest.mark.parametrize("n", [4096, 8192])  # powers of two: the one-launch paths, and the general sort and accumulation
def test_evaluation_form_submits_read_only(engines, oracle, n):
    """kzg_commit_evaluations_submit, kzg_commit_lagrange_submit and kzg_open_lagrange_submit on one region of values"""
    e = engines.bench_srs(8193)
    evals, coeffs = _evals_case(n)
    z = _rand(1, 71)[0]
    y = TO.poly_eval(coeffs, z)
    ar, d, _ = _read_only(e, n, values=[evals])
    with ar:
        e.commit_evaluations_submit(0, d.ptr, n)
        assert e.wait(0).compress() == TO.commitment(oracle, coeffs, S)
        ar.check_untouched()
        e.lagrange_prepare(NO.log2_exact(n))
        e.commit_lagrange_submit(0, d.ptr, n)
        assert e.wait(0).compress() == TO.g1_scalar(oracle, NO.barycentric_eval(evals, S))
        ar.check_untouched()
        e.open_lagrange_submit(0, d.ptr, n, K.Scalar(z), K.Scalar(y))
        assert e.wait(0).compress() == TO.proof(oracle, coeffs, z, S, y)
        ar.check_untouched()


# ---- error returns: the status is the documented one; inputs, guards and gaps are intact; the output is left open -----------------
def test_zero_denominators_leave_everything_but_the_output(eng):
    n, t = 2 * GP_TILE + 1, 3
    nums, dens = _cols(n, t, 2), [list(c) for c in _cols(n, t, 3, low=1)]
    dens[2][2 * GP_TILE], dens[0][GP_TILE - 1] = 0, 0  # two tiles: the least index is reported
    ar, d_a, d_z, d_b = _gp_arena(eng, nums, dens, n, t)
    with ar:
        err = _raises(K.KZG_ERR_INVALID_ARG, lambda: eng.grand_product_device(d_a.ptr, d_b.ptr, n, t, d_z.ptr, stride=n + 5))
        assert err.bad_index == GP_TILE - 1
        ar.check(unasserted=[d_z])
    n = 2 * LU_TILE + 1
    dens = [list(c) for c in _cols(n, t, 7, low=1)]
    dens[1][2 * LU_TILE], dens[2][LU_TILE] = 0, 0
    with DA.Arena(eng, seed=n) as ar:
        d_phi = ar.region(n, name="phi")
        d_b = ar.region(n, t, n + 5, name="dens", data=_lim(dens))
        ar.upload()
        err = _raises(K.KZG_ERR_INVALID_ARG, lambda: eng.logderivative_sum_device(None, d_b.ptr, n, t, d_phi.ptr, stride=n + 5))
        assert err.bad_index == LU_TILE
        ar.check(unasserted=[d_phi])


def test_a_value_in_no_table_row_leaves_everything_but_the_outputs(eng):
    n_table, n, k = 257, 257, 3
    table = TL._table(n_table)
    lookups = [list(col) for col in TL._draw(table, n, k, n_table + n)]
    lookups[2][200], lookups[0][256] = TL._table(n_table, 1)[0], TL._table(n_table, 1)[1]
    assert LO.multiplicities(table, lookups)[2] == 200
    with DA.Arena(eng, seed=3) as ar:
        d_t = ar.region(n_table, name="table", data=LO.to_limbs(table))
        d_m = ar.region(n_table, name="mult")
        d_f = ar.region(n, k, n + 5, name="lookups", data=_lim(lookups))
        d_r = ar.region(n, k, name="rows", row_bytes=4)
        ar.upload()
        err = _raises(K.KZG_ERR_INVALID_ARG, lambda: eng.lookup_multiplicities_device(d_t.ptr, n_table, d_f.ptr, n, k, d_m.ptr, d_r.ptr,
                                                                                    stride=n + 5))
        assert err.bad_index == 200
        ar.check(unasserted=[d_m, d_r])


def test_remainders_leave_everything_but_the_output(eng, engines):
    n, e = 512, 4
    N = n * e
    T, num, _ = _vq_case(n, e)
    with DA.Arena(eng, seed=4) as ar:
        d_in = ar.region(N, name="num", data=GO.to_limbs([(v + 1) % R for v in num]))
        d_out = ar.region(N - n, name="T")
        ar.upload()
        _raises(K.KZG_ERR_REMAINDER, lambda: eng.vanishing_quotient_device(d_in.ptr, N, n, d_out.ptr))
        ar.check(unasserted=[d_out])
    n, t, log_ext = 256, 3, 2
    N = n << log_ext
    eg = engines.bench_srs(TCO.SRS)
    c, z, T, coefs = TCO._case(n, t, True)
    wires = [list(col) for col in c.wires]
    wires[0][3] = (wires[0][3] + 1) % R  # the gate does not hold at row 3
    circ = TCO._create(eg, c, log_ext)
    try:
        with DA.Arena(eg, seed=5) as ar:
            d_w = ar.region(n, t, n + 5, name="wires", data=_lim(wires))
            d_t = ar.region(N - n, name="T")
            d_z = ar.region(n, name="z", data=GO.to_limbs(z))
            d_pi = ar.region(n, name="pi", data=GO.to_limbs(c.pi))
            ar.upload()
            _raises(K.KZG_ERR_REMAINDER, lambda: circ.quotient_device(d_w.ptr, d_z.ptr, *TCO._ch()[:3], d_t.ptr, d_public_inputs=d_pi.ptr,
                                                                    stride=n + 5))
            ar.check(unasserted=[d_t])
    finally:
        circ.close()


def test_overlap_refusals_touch_nothing(eng):
    n, t = GP_TILE + 1, 3
    nums, dens = _cols(n, t, 2), _cols(n, t, 3, low=1)
    ar, d_a, d_z, d_b = _gp_arena(eng, nums, dens, n, t)
    with ar:
        # the output inside the denominators' last column, and starting in the gap after the numerators' first
        # INVALID_ARG is also what a wrong shape returns: kzg_last_error says that this refusal is about the overlap
        def refused(call):
            _raises(K.KZG_ERR_INVALID_ARG, call)
            assert b"overlaps" in eng._lib.kzg_last_error(eng._h)
        for out in (d_b.col_ptr(t - 1) + 64, d_a.ptr + n * 32):
            refused(lambda: eng.grand_product_device(d_a.ptr, d_b.ptr, n, t, out, stride=n + 5))
        eng.coset_extend_device(d_a.ptr, 4, 1, 3, d_z.ptr)  # the shape itself is accepted (4 values -> 8 in the output region) ..
        refused(lambda: eng.coset_extend_device(d_a.ptr, 4, 1, 3, d_a.ptr + 64))  # .. and refused two rows into its input
        refused(lambda: eng.vanishing_quotient_device(d_a.ptr, 8, 2, d_a.ptr + 7 * 32))
        ar.check(unasserted=[d_z])


# ---- host forms whose output length is not the obvious one: only the documented range of a larger buffer changes -----------------
def _filled(nbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, size=nbytes, dtype=np.uint8)


def _only_changed(buf, fill, nbytes, want):
    """the first nbytes of buf are `want`, the rest is the fill"""
    assert np.array_equal(buf[:nbytes], np.ascontiguousarray(want).view(np.uint8).reshape(-1)), "the documented range"
    changed = np.flatnonzero(buf[nbytes:] != fill[nbytes:])
    assert changed.size == 0, "byte %d past the documented end was written (%d in all)" % (int(changed[0]), changed.size)


def test_host_vanishing_quotient_writes_n_rows_less(eng):
    n, e = 512, 4
    N = n * e
    T, num, _ = _vq_case(n, e)
    a = GO.to_limbs(num)
    fill = _filled((N + 64) * 32, 1)
    out = fill.copy()
    assert eng._lib.kzg_vanishing_quotient(eng._h, a.ctypes.data, N, n, 0, out.ctypes.data) == K.KZG_OK
    _only_changed(out, fill, (N - n) * 32, GO.to_limbs(T))
    assert np.array_equal(a, GO.to_limbs(num))


def test_host_coset_extend_writes_batch_times_N(eng):
    length, batch, log_N = 3, 3, 8
    N = 1 << log_N
    cols = [_rand(length, 20 + j) for j in range(batch)]
    want = _lim([_memo(("ext", N, "coeffs_3", j), lambda j=j: (cols[j], PQ.coset_extend(cols[j], log_N)))[1] for j in range(batch)])
    a = np.ascontiguousarray(_lim(cols))
    fill = _filled((batch * N + 64) * 32, 2)
    out = fill.copy()
    assert eng._lib.kzg_coset_extend(eng._h, a.ctypes.data, length, batch, length, K.KZG_EXTEND_COEFFS, log_N, out.ctypes.data) == K.KZG_OK
    _only_changed(out, fill, batch * N * 32, want)


def test_host_lookup_multiplicities_writes_k_n_words(eng):
    n_table, n, k = 257, 257, 3
    table = TL._table(n_table)
    lookups = TL._draw(table, n, k, n_table + n)
    counts, rows, _ = LO.multiplicities(table, lookups)
    tb, f = LO.to_limbs(table), np.ascontiguousarray(_lim(lookups))
    fill_m, fill_r = _filled((n_table + 8) * 32, 3), _filled(k * n * 4 + 256, 4)
    mult, out_rows, bad = fill_m.copy(), fill_r.copy(), C.c_size_t(0)
    assert eng._lib.kzg_lookup_multiplicities(eng._h, tb.ctypes.data, n_table, f.ctypes.data, n, k, n, mult.ctypes.data,
                                              out_rows.ctypes.data, C.byref(bad)) == K.KZG_OK
    assert bad.value == NONE
    _only_changed(mult, fill_m, n_table * 32, LO.to_limbs(counts))
    _only_changed(out_rows, fill_r, k * n * 4, np.array(rows, dtype=np.uint32))


def _check_quotient_outputs(oracle, n, log_ext, T, coeffs, fill_c, p1s, fill_p):
    N, chunks = n << log_ext, (1 << log_ext) - 1
    full = list(T) + [0] * (N - n - len(T))
    _only_changed(coeffs, fill_c, (N - n) * 32, GO.to_limbs(full))
    points = p1s[:chunks * 144].view(np.uint64).reshape(chunks, 18)
    for c in range(chunks):
        assert K.G1Point(points[c].copy()).compress() == TO.g1_scalar(oracle, PQ.horner(full[c * n:(c + 1) * n], S)), c
    changed = np.flatnonzero(p1s[chunks * 144:] != fill_p[chunks * 144:])
    assert changed.size == 0, "out_p1s: byte %d past chunk %d was written" % (int(changed[0]), chunks - 1)


def test_host_quotients_write_N_minus_n_coefficients_and_one_point_per_chunk(engines, oracle):
    """kzg_circuit_quotient and, on the same circuit's wires and sigmas with the gate handed in, kzg_permutation_quotient"""
    n, t, log_ext = 256, 3, 2
    N = n << log_ext
    e = engines.bench_srs(TCO.SRS)
    c, z, T, coefs = TCO._case(n, t, True)
    w, zz, pi = np.ascontiguousarray(_lim(c.wires)), GO.to_limbs(z), GO.to_limbs(c.pi)
    ch = [x.limbs() for x in TCO._ch()[:3]]
    p = lambda x: x.ctypes.data
    fill_c, fill_p = _filled(N * 32 + 96, 5), _filled((1 << log_ext) * 144 + 64, 6)
    circ = TCO._create(e, c, log_ext)
    try:
        coeffs, p1s = fill_c.copy(), fill_p.copy()
        assert e._lib.kzg_circuit_quotient(e._h, circ._c, p(w), n, p(zz), p(pi), p(ch[0]), p(ch[1]), p(ch[2]), None, p(coeffs),
                                           p(p1s)) == K.KZG_OK
        _check_quotient_outputs(oracle, n, log_ext, T, coeffs, fill_c, p1s, fill_p)
    finally:
        circ.close()
    # the permutation quotient of the same argument alone (G = 0) divides as well: the wires are constant on the cycles
    ks = c.ks
    zp, last = PQ.z_of(c.wires, c.sigmas, ks, BETA, GAMMA)
    assert last == 1
    Tp = _memo(("pq_T", n, t), lambda: PQ.quotient(c.wires, c.sigmas, zp, ks, ALPHA, BETA, GAMMA))
    s, sh, zl = np.ascontiguousarray(_lim(c.sigmas)), GO.to_limbs(ks), GO.to_limbs(zp)
    coeffs, p1s = fill_c.copy(), fill_p.copy()
    assert e._lib.kzg_permutation_quotient(e._h, p(w), p(s), p(zl), n, t, n, p(sh), p(ch[0]), p(ch[1]), p(ch[2]), None, log_ext,
                                           p(coeffs), p(p1s)) == K.KZG_OK
    _check_quotient_outputs(oracle, n, log_ext, Tp, coeffs, fill_c, p1s, fill_p)
