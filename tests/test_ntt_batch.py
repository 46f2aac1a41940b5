"""CPU: what kzg_ntt_batch / kzg_ntt_batch_device answer before any device is touched, and that header, wrapper and library
agree on the two names.  The context is a zeroed block that is never read past its first word ("not a multi-device context"):
every call here returns from its argument checks."""
import ctypes as C
import os
import re

import numpy as np

import kzg_poly_commit_exploration_amd as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = K.KZG_ERR_INVALID_ARG


def _calls():
    lib = K.load_library()

    def host(ctx, src, n, batch, s_in, dst, s_out, inverse=0):
        return lib.kzg_ntt_batch(ctx, C.c_void_p(src), n, batch, s_in, inverse, C.c_void_p(dst), s_out)

    def dev(ctx, src, n, batch, s_in, dst, s_out, inverse=0):
        return lib.kzg_ntt_batch_device(ctx, C.c_void_p(src), n, batch, s_in, C.c_void_p(dst), s_out, inverse)

    return host, dev


def test_argument_errors_without_a_device():
    block = np.zeros(1 << 16, dtype=np.uint8)
    ctx = block.ctypes.data
    a = np.zeros((3, 40, 4), dtype=np.uint64)
    out = np.zeros((3, 40, 4), dtype=np.uint64)
    pa, po, n, batch, stride = a.ctypes.data, out.ctypes.data, 32, 3, 40
    for call in _calls():
        assert call(None, pa, n, batch, stride, po, stride) == INV
        assert call(ctx, None, n, batch, stride, po, stride) == INV
        assert call(ctx, pa, n, batch, stride, None, stride) == INV
        for bad_n in (0, 3, 6, 1000, (1 << 22) + 1, 1 << 23):  # kzg_ntt's sizes
            assert call(ctx, pa, bad_n, batch, 1 << 24, po, 1 << 24) == INV, bad_n
        assert call(ctx, pa, n, batch, n - 1, po, stride) == INV  # strides below n
        assert call(ctx, pa, n, batch, stride, po, n - 1) == INV
        assert call(ctx, pa, n, batch, 1 << 62, po, stride) == INV  # extents beyond the address space
        assert call(ctx, pa, n, batch, stride, po, 1 << 62) == INV
        # overlap: only the same base with equal strides is allowed
        assert call(ctx, pa, n, batch, stride, pa, stride + 1) == INV
        assert call(ctx, pa, n, batch, stride, pa + 32, stride) == INV
        assert call(ctx, pa, n, batch, stride, pa + 32 * stride, stride) == INV
        assert call(ctx, pa, n, batch, stride, pa - 32, stride) == INV
        assert call(ctx, pa + 32 * (stride * (batch - 1) + n - 1), n, batch, stride, pa, stride) == INV  # the last value of the output
        # an empty batch does nothing, whatever the two sides share
        assert call(ctx, pa, n, 0, stride, po, stride) == 0
        assert call(ctx, pa, n, 0, stride, pa + 32, stride, 1) == 0
        assert call(ctx, pa, 6, 0, stride, po, stride) == INV  # ... but its shape is still checked
    assert not block.any() and not a.any() and not out.any()


def test_header_wrapper_and_library_agree():
    lib = K.load_library()
    header = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    for name in ("kzg_ntt_batch", "kzg_ntt_batch_device", "kzg_ntt_batch_rounds"):
        assert re.search(r"\bint %s\(kzg_ctx\* ctx," % name, header), name
        assert name in K.ABI_SYMBOLS and hasattr(lib, name)
    assert hasattr(K.Engine, "ntt_batch_limbs") and hasattr(K.Engine, "ntt_batch_device")
