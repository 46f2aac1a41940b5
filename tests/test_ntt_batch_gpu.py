"""GPU: kzg_ntt_batch / kzg_ntt_batch_device (ntt_batch_kernels.hip: k_nttb_pass) bit for bit against kzg_ntt of every column,
and against the big-integer transforms of tests/ntt_oracle.py up to one tile.

The sizes are the smallest at which the launches differ: 2^0, 2^1, 2^5 (one workgroup per column, a partial tile), 2^11 (one
full tile), 2^12 (two passes, 6 + 6), 2^13 (7 + 6: unequal radices), 2^19 (three passes, 7 + 6 + 6).  Batches of 1, 2, 3 and 5
columns (2 at 2^19), input stride n + 5 and output stride n + 3 with the rows between the columns filled and required unchanged,
in place with equal strides, the device form inside the guard bands of tests/device_arena.py, a workspace budget under which five
columns of 2^12 values take three rounds, and every argument error with the context serving afterwards."""
import ctypes as C

import numpy as np
import pytest

import device_arena as DA
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO

pytestmark = pytest.mark.gpu
R = NO.R
LOGS = [0, 1, 5, 11, 12, 13, 19]
IN_GAP, OUT_GAP = 5, 3
_CACHE = {}  # references computed once, shared and left unchanged


@pytest.fixture(scope="module")
def eng():
    e = K.Engine(0)  # no SRS: the transform needs none
    yield e
    e.close()


def _batches(k):
    return [2] if k == 19 else [1, 2, 3, 5]


def _images(shape, seed):
    """random blst_fr images below r (top limb below r's): canonical"""
    c = np.random.default_rng(seed).integers(0, 2**64, size=tuple(shape) + (4,), dtype=np.uint64, endpoint=False)
    c[..., 3] %= np.uint64(R >> 192)
    return c


def _columns(k):
    """the widest batch of size 2^k at the input stride, gaps filled: (batch, n + 5, 4)"""
    if ("in", k) not in _CACHE:
        a = _images((max(_batches(k)), (1 << k) + IN_GAP), 100 + k)
        a.setflags(write=False)
        _CACHE[("in", k)] = a
    return _CACHE[("in", k)]


def _want(eng, k, inverse):
    """kzg_ntt of every column: (batch, n, 4)"""
    key = ("want", k, inverse)
    if key not in _CACHE:
        n = 1 << k
        w = np.stack([eng.intt_limbs(col[:n]) if inverse else eng.ntt_limbs(col[:n]) for col in _columns(k)])
        w.setflags(write=False)
        _CACHE[key] = w
    return _CACHE[key]


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("k", LOGS)
def test_host_form_matches_ntt_per_column(eng, k, inverse):
    n = 1 << k
    want = _want(eng, k, inverse)
    for batch in _batches(k):
        a = _columns(k)[:batch].copy()
        fill = _images((batch, n + OUT_GAP), 7 * k + batch)
        out = fill.copy()
        assert eng.ntt_batch_limbs(a, n, inverse, out=out) is out
        assert np.array_equal(out[:, :n], want[:batch]), (k, batch, inverse)
        assert np.array_equal(out[:, n:], fill[:, n:]), (k, batch, "rows between the output columns")
        assert np.array_equal(a, _columns(k)[:batch]), (k, batch, "the input")
        # a new packed array
        assert np.array_equal(eng.ntt_batch_limbs(a, n, inverse), want[:batch]), (k, batch, inverse, "packed")
        # in place, equal strides
        eng.ntt_batch_limbs(a, n, inverse, out=a)
        assert np.array_equal(a[:, :n], want[:batch]), (k, batch, inverse, "in place")
        assert np.array_equal(a[:, n:], _columns(k)[:batch, n:]), (k, batch, "rows between the columns, in place")


@pytest.mark.parametrize("k", [0, 1, 5, 11])
def test_matches_the_big_integer_oracle(eng, k):
    n = 1 << k
    a = _columns(k)
    got_f, got_i = eng.ntt_batch_limbs(a, n, False), eng.ntt_batch_limbs(a, n, True)
    for b in range(a.shape[0]):
        v = K.limbs_to_scalars(a[b, :n])
        assert K.limbs_to_scalars(got_f[b]) == NO.ntt(v), (k, b, "forward")
        assert K.limbs_to_scalars(got_i[b]) == NO.intt(v), (k, b, "inverse")


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("k", LOGS)
def test_device_form_inside_guard_bands(eng, k, inverse):
    n = 1 << k
    want = _want(eng, k, inverse)
    for batch in _batches(k):
        cols = _columns(k)[:batch, :n]
        with DA.Arena(eng, seed=31 * k + batch) as arena:
            src = arena.region(n, batch, n + IN_GAP, "in", data=cols)
            dst = arena.region(n, batch, n + OUT_GAP, "out")
            both = arena.region(n, batch, n + IN_GAP, "in place", data=cols)
            arena.upload()
            eng.ntt_batch_device(src.ptr, n, batch, n + IN_GAP, dst.ptr, n + OUT_GAP, inverse)
            eng.ntt_batch_device(both.ptr, n, batch, n + IN_GAP, both.ptr, n + IN_GAP, inverse)
            arena.check({dst: want[:batch], both: want[:batch]})


def test_rounds_under_a_small_budget(eng, monkeypatch):
    """KZG_PQ_WS_KB = 1024 (read when a context is created): a quarter of it holds two columns of 2^12 values, so five columns
    take rounds of 2, 2 and 1; 2^13 values take one column per round"""
    monkeypatch.setenv("KZG_PQ_WS_KB", "1024")
    small = K.Engine(0)
    try:
        assert [small.ntt_batch_rounds(1 << 12, b) for b in (0, 1, 2, 3, 5)] == [0, 1, 1, 2, 3] and small.ntt_batch_rounds(1 << 13, 5) == 5
        assert [eng.ntt_batch_rounds(1 << 12, b) for b in (0, 1, 5, 64, 65)] == [0, 1, 1, 1, 2] and eng.ntt_batch_rounds(1 << 13, 5) == 1
        for k, inverse in ((12, False), (12, True), (13, False)):
            n, want = 1 << k, _want(eng, k, inverse)
            a = _columns(k)
            fill = _images((a.shape[0], n + OUT_GAP), k)
            out = fill.copy()
            small.ntt_batch_limbs(a, n, inverse, out=out)
            assert np.array_equal(out[:, :n], want) and np.array_equal(out[:, n:], fill[:, n:]), (k, inverse)
            with DA.Arena(small, seed=k) as arena:
                src = arena.region(n, a.shape[0], n + IN_GAP, "in", data=a[:, :n])
                dst = arena.region(n, a.shape[0], n + OUT_GAP, "out")
                arena.upload()
                small.ntt_batch_device(src.ptr, n, a.shape[0], n + IN_GAP, dst.ptr, n + OUT_GAP, inverse)
                arena.check({dst: want})
    finally:
        small.close()


def test_multi_device_context(eng):
    """the host form runs on the first device; the device form takes single-device contexts"""
    k, n = 12, 1 << 12
    multi = K.Engine(devices=[0, 0])
    try:
        assert np.array_equal(multi.ntt_batch_limbs(_columns(k), n, True), _want(eng, k, True))
        lib = K.load_library()
        rc = lib.kzg_ntt_batch_device(multi._h, C.c_void_p(32), n, 1, n, C.c_void_p(32), n, 0)
        assert rc == K.KZG_ERR_INVALID_ARG
    finally:
        multi.close()


def test_argument_errors_leave_the_context_serving(eng):
    lib = K.load_library()
    k, n, batch = 5, 32, 3
    a = _columns(k)[:batch].copy()
    stride = a.shape[1]
    out = np.zeros_like(a)
    before = out.copy()
    INV = K.KZG_ERR_INVALID_ARG

    def host(ctx, src, n_, batch_, s_in, dst, s_out):
        return lib.kzg_ntt_batch(ctx, C.c_void_p(src), n_, batch_, s_in, 0, C.c_void_p(dst), s_out)

    def dev(ctx, src, n_, batch_, s_in, dst, s_out):
        return lib.kzg_ntt_batch_device(ctx, C.c_void_p(src), n_, batch_, s_in, C.c_void_p(dst), s_out, 0)

    pa, po = a.ctypes.data, out.ctypes.data
    for call in (host, dev):
        assert call(None, pa, n, batch, stride, po, stride) == INV
        assert call(eng._h, None, n, batch, stride, po, stride) == INV
        assert call(eng._h, pa, n, batch, stride, None, stride) == INV
        for bad_n in (0, 3, 6, 1000, (1 << 22) + 1, 1 << 23):
            assert call(eng._h, pa, bad_n, batch, 1 << 24, po, 1 << 24) == INV, bad_n
        assert call(eng._h, pa, n, batch, n - 1, po, stride) == INV  # a stride below n
        assert call(eng._h, pa, n, batch, stride, po, n - 1) == INV
        assert call(eng._h, pa, n, batch, 1 << 62, po, stride) == INV  # an extent beyond the address space
        assert call(eng._h, pa, n, batch, stride, pa, stride + 1) == INV  # the same base, unequal strides
        assert call(eng._h, pa, n, batch, stride, pa + 32, stride) == INV  # shifted by one value
        assert call(eng._h, pa, n, batch, stride, pa + 32 * stride, stride) == INV  # shifted by one column
        assert call(eng._h, pa + 32 * (stride * (batch - 1) + n - 1), n, batch, stride, pa, stride) == INV  # the last value of the output
        assert call(eng._h, pa, n, 0, stride, po, stride) == 0  # an empty batch does nothing
        assert call(eng._h, pa, n, 0, stride, pa + 32, stride) == 0
    assert np.array_equal(out, before) and np.array_equal(a, _columns(k)[:batch])
    assert np.array_equal(eng.ntt_batch_limbs(a, n), _want(eng, k, False)[:batch])
    # adjacent, not overlapping: the output starts where the input ends
    flat = np.concatenate([a[0, :n], np.zeros((n, 4), dtype=np.uint64)])
    assert host(eng._h, flat.ctypes.data, n, 1, n, flat.ctypes.data + 32 * n, n) == 0
    assert np.array_equal(flat[n:], _want(eng, k, False)[0]) and np.array_equal(flat[:n], a[0, :n])
