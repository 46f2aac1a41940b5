"""CPU: what kzg_circuit_prove / kzg_circuit_prove_device answer before any device is touched (a zeroed block as the context: only
its first word, "not a multi-device context", is read), and that header, wrapper and library agree on the two names.  The proofs
themselves are tests/test_circuit_prove_gpu.py's; the transcript and the verifier are tests/test_circuit_proof.py's."""
import ctypes as C
import os
import re

import numpy as np

import kzg_poly_commit_exploration_amd as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = K.KZG_ERR_INVALID_ARG


def test_null_pointers_are_refused_before_the_context_is_read():
    lib = K.load_library()
    block = np.zeros(1 << 16, dtype=np.uint8)
    ctx = block.ctypes.data
    a = np.zeros((64, 4), dtype=np.uint64)
    out = np.full(576, 0x5A, dtype=np.uint8)
    p, o = a.ctypes.data, out.ctypes.data
    good = [ctx, p, p, p, 8, p, 2, p, o]  # ctx, circuit, key, wires, stride, public inputs, n_public, blinders, out_proof
    for fn in (lib.kzg_circuit_prove, lib.kzg_circuit_prove_device):
        for pos in (0, 1, 2, 3, 8):
            args = list(good)
            args[pos] = None
            assert fn(*args) == INV, pos
        args = list(good)
        args[5] = None  # public inputs may be NULL only when there are none
        assert fn(*args) == INV
    assert (out == 0x5A).all() and not block.any()


def test_header_wrapper_and_library_agree():
    lib = K.load_library()
    header = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    for name in ("kzg_circuit_prove", "kzg_circuit_prove_device"):
        assert re.search(r"\bint %s\(kzg_ctx\* ctx, const kzg_circuit\* circuit," % name, header), name
        assert name in K.ABI_SYMBOLS and hasattr(lib, name)
    assert callable(K.Circuit.prove) and callable(K.Circuit.prove_device)
