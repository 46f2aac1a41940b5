"""Satisfied circuits with their proofs from tests/transcript_oracle.py, for tests that feed the same case to more than one
interface (tests/test_hpp_parity_gpu.py: the C++ header and the Python mirror).  The seeds are those of
tests/test_circuit_proof_gpu.py, so the cases are the ones that module proves through the C-ABI."""
import numpy as np

import bigint_twin as BT
import blind_oracle as BO
import circuit_oracle as CO
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import transcript_oracle as TR

S = BT.fr_from_be_bytes(BT.BENCH_SECRET_BE)
_CACHE = {}  # references computed once, shared and left unchanged


def case(oracle, n, t, log_ext, with_pi, blinded, seed=0):
    """(the blinders, transcript_oracle.prove's dict) of a satisfied circuit of n rows and t columns under the bench secret"""
    key = (n, t, log_ext, with_pi, blinded, seed)
    if key not in _CACHE:
        c = CO.satisfied(NO.log2_exact(n), t, 900 + n + t, with_pi)
        bl = BO.Blinders.random(t, log_ext, 10 * seed + n + t) if blinded else BO.Blinders.zero(t, log_ext)
        _CACHE[key] = (bl, TR.prove(oracle, c, log_ext, bl, S))
    return _CACHE[key]


def limbs(cols, stride):
    """columns -> (t, stride, 4) blst_fr rows; the rows past n hold values that are not the columns'"""
    n = len(cols[0])
    out = np.empty((len(cols), stride, 4), dtype=np.uint64)
    for j, col in enumerate(cols):
        out[j] = GO.to_limbs(list(col) + [0xBAD + i for i in range(stride - n)])
    return out


def create(e, c, log_ext):
    """the circuit on engine e through the Python mirror, with its key"""
    return e.circuit_create(limbs(c.q_lin, c.n + 3), GO.to_limbs(c.q_mul), GO.to_limbs(c.q_const), limbs(c.sigmas, c.n + 3),
                            [K.Scalar(k) for k in c.ks], log_ext, n=c.n, want_key=True)
