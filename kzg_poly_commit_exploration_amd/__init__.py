"""kzg_poly_commit_exploration_amd -- host-side mirror of the reference's commit / open API over
the MI355X engine (libkzg_mi355x.so, C-ABI in include/kzg_mi355x.h).

The names follow the reference crate (VGLoic/kzg-poly-commit-exploration): Scalar
(src/scalar.rs), G1Point (src/curves.rs), SetupArtifactsGenerator (src/trusted_setup.rs),
Polynomial / Evaluation (src/polynomial.rs) -- same argument meaning, same error messages -- so
the parity tests read like the reference's own tests (src/lib.rs:16-33).  Everything that is
arithmetic on the hot path goes through the C-ABI into HIP kernels; this module only converts
representations (Python ints <-> blst limb layouts), which is what the reference's Rust host code
does around its blst calls.  There is no CPU fallback: importing works without a GPU, creating an
Engine does not.
"""
import ctypes as C
import os

import numpy as np

__all__ = [
    "Engine", "Scalar", "G1Point", "Polynomial", "Evaluation", "SetupArtifactsGenerator", "KzgError",
    "R_MODULUS", "lib_path", "load_library", "ABI_SYMBOLS", "srs_g2_at", "verify_proof", "verify_proof_batch",
    "verify_points", "KZG_MAX_OPEN_POINTS", "KZG_NTT_MAX_LOG", "KZG_GP_MAX_COLUMNS", "KZG_PQ_MAX_COLUMNS", "KZG_LOGUP_MAX_COLUMNS",
    "KZG_PQ_MAX_LOG_EXT", "KZG_EXTEND_VALUES", "KZG_EXTEND_COEFFS", "domain_root",
    "Circuit", "circuit_verify", "circuit_blinders", "circuit_blinded_sizes", "circuit_proof_size", "circuit_proof_challenges", "circuit_verify_proof",
    "KZG_CIRCUIT_MIN_COLUMNS", "KZG_CIRCUIT_COL_QLIN", "KZG_CIRCUIT_COL_QM", "KZG_CIRCUIT_COL_QC", "KZG_CIRCUIT_COL_SIGMA",
    "KZG_CIRCUIT_COL_L0", "KZG_CIRCUIT_VALUES", "KZG_CIRCUIT_COEFFS", "KZG_CIRCUIT_COSET",
    "KZG_CIRCUIT_COL_TABLE", "KZG_CIRCUIT_COL_QLOOKUP",
    "circuit_lookup_proof_size", "circuit_lookup_proof_challenges", "circuit_lookup_verify_proof",
    "circuit_lookup_blinded_sizes", "circuit_lookup_blinders",
    "combine_claims", "verify_combined", "KZG_MAX_COMBINE",
    "verify_sets", "KZG_MAX_SETS", "KZG_MAX_SET_POINTS",
    "ml_verify", "KZG_ML_MAX_VARS",
    "sha256", "sha256_has_shani", "blob_challenges_bytes",
]

_HERE = os.path.dirname(os.path.abspath(__file__))
R_MODULUS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001  # src/scalar.rs:10
_FR_R = 1 << 256
_FR_RINV = pow(_FR_R, -1, R_MODULUS)

KZG_OK = 0
KZG_ERR_DEGREE_TOO_HIGH = -1
KZG_ERR_CONSTANT_POLY = -2
KZG_ERR_REMAINDER = -3
KZG_ERR_INVALID_ARG = -4
KZG_ERR_NO_DEVICE = -5
KZG_ERR_HIP = -6
KZG_ERR_NO_SRS = -7
KZG_ERR_BUSY = -8
KZG_MULTI_REPLICATE_SRS = 1
KZG_ABI_VERSION = 4

# every symbol include/kzg_mi355x.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "kzg_ctx_create", "kzg_ctx_destroy", "kzg_strerror", "kzg_last_error",
    "kzg_srs_load_g1", "kzg_srs_generate_g1", "kzg_srs_read_g1", "kzg_srs_len",
    "kzg_commit", "kzg_commit_le_bytes", "kzg_open", "kzg_quotient", "kzg_evaluate",
    "kzg_srs_load_affine", "kzg_srs_load_compressed", "kzg_srs_save", "kzg_srs_load_file",
    "kzg_ctx_create_multi", "kzg_ctx_create_multi_ex", "kzg_abi_version", "kzg_commit_batch", "kzg_open_batch", "kzg_num_devices", "kzg_rccl_exchanges", "kzg_num_slots", "kzg_commit_submit", "kzg_open_submit", "kzg_wait",
    "kzg_set_max_batch", "kzg_max_batch", "kzg_commit_batch_submit", "kzg_wait_batch",
    "kzg_open_batch_submit", "kzg_wait_open_batch", "kzg_g1_uncompress",
    "kzg_dev_alloc", "kzg_dev_free", "kzg_dev_upload", "kzg_dev_download",
    "kzg_g1_sum", "kzg_g1_compress", "kzg_srs_g2_at", "kzg_verify_proof", "kzg_verify_proof_batch", "kzg_set_timing", "kzg_get_times", "kzg_msm_config",
    "kzg_open_points", "kzg_open_points_submit", "kzg_quotient_points", "kzg_evaluate_points", "kzg_verify_points",
    "kzg_domain_root", "kzg_ntt", "kzg_ntt_device", "kzg_commit_evaluations", "kzg_commit_evaluations_submit",
    "kzg_open_evaluations", "kzg_cells_and_proofs", "kzg_cells_and_proofs_evaluations", "kzg_quotient_cells",
    "kzg_cells_and_proofs_fk20", "kzg_fk20_prepare", "kzg_g1_dft", "kzg_recover_cells_and_proofs",
    "kzg_verify_cells_batch", "kzg_verify_cells_lincomb",
    "kzg_evaluate_evaluations_batch", "kzg_verify_openings_batch", "kzg_verify_openings_lincomb", "kzg_verify_evaluations_batch",
    "kzg_verify_cells_batch_bytes", "kzg_verify_cells_lincomb_bytes", "kzg_verify_openings_batch_bytes",
    "kzg_verify_openings_lincomb_bytes", "kzg_verify_blobs_batch_bytes", "kzg_g1_uncompress_batch", "kzg_fr_from_bytes_batch",
    "kzg_blobs_to_commitments_bytes", "kzg_blobs_to_cells_and_proofs_bytes", "kzg_recover_cells_and_proofs_bytes",
    "kzg_g1_compress_batch", "kzg_fr_to_bytes_batch",
    "kzg_srs_update", "kzg_srs_verify", "kzg_srs_verify_lincomb", "kzg_g2_mul", "kzg_srs_verify_update",
    "kzg_open_combined", "kzg_open_combined_submit", "kzg_wait_combined", "kzg_get_combine_ms", "kzg_combine_polys",
    "kzg_evaluate_batch_at", "kzg_combine_claims", "kzg_verify_combined",
    "kzg_open_sets", "kzg_open_sets_submit", "kzg_wait_sets", "kzg_quotient_sets", "kzg_verify_sets",
    "kzg_sha256", "kzg_sha256_pieces", "kzg_sha256_has_shani", "kzg_blob_challenges_bytes", "kzg_blobs_open_at_bytes", "kzg_blobs_to_blob_proofs_bytes",
    "kzg_verify_blob_proofs_batch_bytes",
    "kzg_lagrange_prepare", "kzg_lagrange_len", "kzg_lagrange_read_g1", "kzg_lagrange_load_compressed",
    "kzg_srs_load_lagrange_compressed", "kzg_commit_lagrange", "kzg_commit_lagrange_submit", "kzg_commit_lagrange_batch",
    "kzg_open_lagrange", "kzg_open_lagrange_submit", "kzg_quotient_lagrange",
    "kzg_grand_product", "kzg_grand_product_device", "kzg_permutation_product", "kzg_permutation_product_device",
    "kzg_permutation_commit",
    "kzg_logderivative_sum", "kzg_logderivative_sum_device", "kzg_lookup_sum", "kzg_lookup_sum_device", "kzg_lookup_commit",
    "kzg_batch_inverse", "kzg_batch_inverse_device", "kzg_lookup_multiplicities", "kzg_lookup_multiplicities_device",
    "kzg_lookup_multiplicities_cap",
    "kzg_coset_extend", "kzg_coset_extend_device", "kzg_permutation_constraints_coset", "kzg_permutation_constraints_coset_device",
    "kzg_vanishing_quotient", "kzg_vanishing_quotient_device", "kzg_permutation_quotient",
    "kzg_circuit_create", "kzg_circuit_destroy", "kzg_circuit_quotient", "kzg_circuit_quotient_device", "kzg_circuit_column_device",
    "kzg_circuit_open", "kzg_circuit_open_device", "kzg_circuit_linearise", "kzg_circuit_verify",
    "kzg_circuit_blinded_sizes", "kzg_circuit_blinders", "kzg_blind_evaluations", "kzg_commit_evaluations_blinded",
    "kzg_circuit_quotient_blinded", "kzg_circuit_quotient_blinded_device", "kzg_circuit_open_blinded",
    "kzg_circuit_open_blinded_device",
    "kzg_ntt_batch", "kzg_ntt_batch_device", "kzg_ntt_batch_rounds",
    "kzg_circuit_proof_size", "kzg_circuit_proof_challenges", "kzg_circuit_verify_proof",
    "kzg_circuit_prove", "kzg_circuit_prove_device",
    "kzg_circuit_create_lookup", "kzg_circuit_lookup_columns", "kzg_circuit_lookup_quotient",
    "kzg_circuit_lookup_prove", "kzg_circuit_lookup_prove_device", "kzg_circuit_lookup_proof_size",
    "kzg_circuit_lookup_proof_challenges", "kzg_circuit_lookup_verify_proof",
    "kzg_circuit_lookup_blinded_sizes", "kzg_circuit_lookup_blinders", "kzg_circuit_lookup_quotient_blinded",
    "kzg_circuit_lookup_prove_blinded", "kzg_circuit_lookup_prove_blinded_device",
    "kzg_circuit_create_custom", "kzg_circuit_custom_gate", "kzg_circuit_custom_quotient", "kzg_circuit_custom_prove",
    "kzg_circuit_custom_prove_device", "kzg_circuit_custom_proof_challenges", "kzg_circuit_custom_verify_proof",
    "kzg_circuit_custom_blinded_sizes",
    "kzg_circuit_create_custom_next", "kzg_circuit_custom_next_gate", "kzg_circuit_custom_next_quotient",
    "kzg_circuit_custom_next_prove", "kzg_circuit_custom_next_prove_device", "kzg_circuit_custom_next_proof_size",
    "kzg_circuit_custom_next_proof_challenges", "kzg_circuit_custom_next_verify_proof",
    "kzg_circuit_verify_proofs_batch", "kzg_circuit_verify_proofs_lincomb", "kzg_circuit_verify_proofs_lincomb_challenges",
    "kzg_ml_fold", "kzg_ml_evaluate", "kzg_ml_fold_device", "kzg_ml_commit_folds_device", "kzg_ml_evaluations_device",
    "kzg_ml_open_device", "kzg_ml_open", "kzg_ml_verify",
]
KZG_VERIFY_MAX_PROOFS = 1 << 16
KZG_SRS_FIRST_IS_GENERATOR = 1
KZG_SRS_OK, KZG_SRS_G2_BAD, KZG_SRS_INFINITY, KZG_SRS_NOT_IN_G1, KZG_SRS_FIRST_NOT_GENERATOR, KZG_SRS_NOT_POWERS = range(6)
KZG_ORDER_NATURAL = 0
KZG_ORDER_BIT_REVERSED = 1
KZG_MAX_OPEN_POINTS = 64
KZG_MAX_COMBINE = 256
KZG_MAX_SETS = 8
KZG_MAX_SET_POINTS = 16
KZG_ML_MAX_VARS = 22  # variables of a multilinear opening (2^22 values: the largest SRS)
KZG_NTT_MAX_LOG = 22
KZG_GP_MAX_COLUMNS = 16  # columns per side of a grand product
KZG_LOGUP_MAX_COLUMNS = 16  # columns per side of a log-derivative sum (a lookup: k <= 15 lookup columns and the table)
KZG_PQ_MAX_COLUMNS = 7   # wire columns of a permutation quotient (t + 1 <= 2^KZG_PQ_MAX_LOG_EXT)
KZG_PQ_MAX_LOG_EXT = 3
KZG_EXTEND_VALUES, KZG_EXTEND_COEFFS = 0, 1
KZG_CIRCUIT_MIN_COLUMNS = 2  # wire columns of a circuit with the built-in arithmetic gate (f_0 f_1 needs two)
KZG_CIRCUIT_COL_QLIN, KZG_CIRCUIT_COL_QM, KZG_CIRCUIT_COL_QC, KZG_CIRCUIT_COL_SIGMA, KZG_CIRCUIT_COL_L0 = 0, 16, 17, 32, 48
KZG_CIRCUIT_VALUES, KZG_CIRCUIT_COEFFS, KZG_CIRCUIT_COSET = 0, 1, 2
KZG_CIRCUIT_COL_TABLE, KZG_CIRCUIT_COL_QLOOKUP = 64, 80  # the columns of a lookup circuit (kzg_circuit_create_lookup)
KZG_CIRCUIT_COL_CUSTOM, KZG_CIRCUIT_MAX_CUSTOM = 96, 8  # the selector columns of a custom circuit (kzg_circuit_create_custom)
KZG_SHA256_AUTO, KZG_SHA256_PORTABLE, KZG_SHA256_SHANI = 0, 1, 2
KZG_MAX_CELL_LOG = 6


class KzgError(Exception):
    """Carries the reference's anyhow message for the three errors of the path."""

    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


class KernelTimes(C.Structure):
    _fields_ = [(n, C.c_float) for n in
                ("digits_ms", "scatter_ms", "accumulate_ms", "reduce_ms", "quotient_ms", "total_ms")
                ] + [("references", C.c_uint64), ("accumulate_events_ms", C.c_float), ("reserved_", C.c_float)]


def lib_path():
    # KZG_MI355X_LIB: another build of the same library (A/B measurements of kernel variants)
    return os.environ.get("KZG_MI355X_LIB") or os.path.join(_HERE, "libkzg_mi355x.so")


_LIB = None


def load_library():
    """Loads the C-ABI library.  Fails loudly if it has not been built (no fallback exists)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(
            "libkzg_mi355x.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  The product has no CPU path.")
    lib = C.CDLL(path)
    vp, sz, u8p, i = C.c_void_p, C.c_size_t, C.c_char_p, C.c_int
    sig = {
        "kzg_ctx_create": (i, [i, C.POINTER(vp)]),
        "kzg_ctx_create_multi": (i, [vp, i, C.POINTER(vp)]),
        "kzg_ctx_create_multi_ex": (i, [vp, i, C.c_uint, C.POINTER(vp)]),
        "kzg_abi_version": (i, []),
        "kzg_commit_batch": (i, [vp, vp, sz, sz, sz, vp]),
        "kzg_open_batch": (i, [vp, vp, sz, sz, sz, vp, vp, vp, vp]),
        "kzg_num_devices": (i, [vp]),
        "kzg_rccl_exchanges": (C.c_uint64, [vp]),
        "kzg_ctx_destroy": (None, [vp]),
        "kzg_strerror": (C.c_char_p, [i]),
        "kzg_last_error": (C.c_char_p, [vp]),
        "kzg_srs_load_g1": (i, [vp, vp, sz, sz]),
        "kzg_srs_generate_g1": (i, [vp, u8p, C.c_uint64, sz]),
        "kzg_srs_read_g1": (i, [vp, sz, sz, vp]),
        "kzg_srs_load_affine": (i, [vp, vp, sz]),
        "kzg_srs_load_compressed": (i, [vp, vp, sz, C.POINTER(sz)]),
        "kzg_srs_save": (i, [vp, C.c_char_p]),
        "kzg_srs_load_file": (i, [vp, C.c_char_p]),
        "kzg_srs_len": (sz, [vp]),
        "kzg_commit": (i, [vp, vp, sz, vp]),
        "kzg_commit_le_bytes": (i, [vp, vp, sz, vp]),
        "kzg_open": (i, [vp, vp, sz, vp, vp, vp]),
        "kzg_quotient": (i, [vp, vp, sz, vp, vp, vp, C.POINTER(sz)]),
        "kzg_evaluate": (i, [vp, vp, sz, vp, vp]),
        "kzg_num_slots": (i, [vp]),
        "kzg_commit_submit": (i, [vp, i, vp, sz]),
        "kzg_open_submit": (i, [vp, i, vp, sz, vp, vp]),
        "kzg_wait": (i, [vp, i, vp]),
        "kzg_set_max_batch": (i, [vp, sz]),
        "kzg_max_batch": (sz, [vp]),
        "kzg_commit_batch_submit": (i, [vp, i, vp, sz, sz, sz]),
        "kzg_wait_batch": (i, [vp, i, vp, sz]),
        "kzg_open_batch_submit": (i, [vp, i, vp, sz, sz, sz, vp, vp]),
        "kzg_wait_open_batch": (i, [vp, i, vp, vp, sz]),
        "kzg_g1_uncompress": (i, [u8p, vp]),
        "kzg_dev_alloc": (i, [vp, sz, C.POINTER(vp)]),
        "kzg_dev_free": (i, [vp, vp]),
        "kzg_dev_upload": (i, [vp, vp, vp, sz]),
        "kzg_dev_download": (i, [vp, vp, vp, sz]),
        "kzg_g1_sum": (i, [vp, sz, vp]),
        "kzg_g1_compress": (i, [vp, vp]),
        "kzg_set_timing": (i, [vp, i]),
        "kzg_get_times": (i, [vp, i, C.POINTER(KernelTimes)]),
        "kzg_srs_g2_at": (i, [u8p, C.c_uint64, vp]),
        "kzg_verify_proof": (i, [vp, vp, vp, vp, vp, C.POINTER(i)]),
        "kzg_verify_proof_batch": (i, [vp, vp, vp, vp, vp, sz, vp]),
        "kzg_msm_config": (i, [vp, C.POINTER(i), C.POINTER(i), C.POINTER(sz), C.POINTER(i)]),
        "kzg_open_points": (i, [vp, vp, sz, vp, vp, sz, vp]),
        "kzg_open_points_submit": (i, [vp, i, vp, sz, vp, vp, sz]),
        "kzg_quotient_points": (i, [vp, vp, sz, vp, vp, sz, vp, C.POINTER(sz)]),
        "kzg_evaluate_points": (i, [vp, vp, sz, vp, sz, vp]),
        "kzg_verify_points": (i, [vp, vp, vp, vp, sz, vp, sz, vp, sz, C.POINTER(i)]),
        "kzg_domain_root": (i, [C.c_uint, vp]),
        "kzg_ntt": (i, [vp, vp, sz, i, vp]),
        "kzg_ntt_device": (i, [vp, vp, vp, sz, i]),
        "kzg_ntt_batch": (i, [vp, vp, sz, sz, sz, i, vp, sz]),
        "kzg_ntt_batch_device": (i, [vp, vp, sz, sz, sz, vp, sz, i]),
        "kzg_ntt_batch_rounds": (i, [vp, sz, sz, C.POINTER(sz)]),
        "kzg_commit_evaluations": (i, [vp, vp, sz, vp]),
        "kzg_commit_evaluations_submit": (i, [vp, i, vp, sz]),
        "kzg_open_evaluations": (i, [vp, vp, sz, vp, vp, vp]),
        "kzg_lagrange_prepare": (i, [vp, C.c_uint]),
        "kzg_lagrange_len": (sz, [vp]),
        "kzg_lagrange_read_g1": (i, [vp, sz, sz, vp]),
        "kzg_lagrange_load_compressed": (i, [vp, vp, sz, C.c_uint, i, C.POINTER(sz), C.POINTER(i)]),
        "kzg_srs_load_lagrange_compressed": (i, [vp, vp, sz, C.c_uint, C.POINTER(sz)]),
        "kzg_commit_lagrange": (i, [vp, vp, sz, vp]),
        "kzg_commit_lagrange_submit": (i, [vp, i, vp, sz]),
        "kzg_commit_lagrange_batch": (i, [vp, vp, sz, sz, sz, vp]),
        "kzg_open_lagrange": (i, [vp, vp, sz, vp, vp, vp]),
        "kzg_open_lagrange_submit": (i, [vp, i, vp, sz, vp, vp]),
        "kzg_quotient_lagrange": (i, [vp, vp, sz, vp, vp, vp]),
        "kzg_grand_product": (i, [vp, vp, vp, sz, sz, sz, vp, vp, C.POINTER(sz)]),
        "kzg_grand_product_device": (i, [vp, vp, vp, sz, sz, sz, vp, vp, C.POINTER(sz)]),
        "kzg_permutation_product": (i, [vp, vp, vp, sz, sz, sz, vp, vp, vp, vp, vp, C.POINTER(sz)]),
        "kzg_permutation_product_device": (i, [vp, vp, vp, sz, sz, sz, vp, vp, vp, vp, vp, C.POINTER(sz)]),
        "kzg_permutation_commit": (i, [vp, vp, vp, sz, sz, sz, vp, vp, vp, vp, vp, vp, C.POINTER(sz)]),
        "kzg_logderivative_sum": (i, [vp, vp, vp, sz, sz, sz, vp, vp, C.POINTER(sz)]),
        "kzg_logderivative_sum_device": (i, [vp, vp, vp, sz, sz, sz, vp, vp, C.POINTER(sz)]),
        "kzg_lookup_sum": (i, [vp, vp, sz, sz, sz, vp, vp, vp, vp, vp, C.POINTER(sz)]),
        "kzg_lookup_sum_device": (i, [vp, vp, sz, sz, sz, vp, vp, vp, vp, vp, C.POINTER(sz)]),
        "kzg_lookup_commit": (i, [vp, vp, sz, sz, sz, vp, vp, vp, vp, vp, vp, C.POINTER(sz)]),
        "kzg_batch_inverse": (i, [vp, vp, sz, vp, C.POINTER(sz)]),
        "kzg_batch_inverse_device": (i, [vp, vp, sz, vp, C.POINTER(sz)]),
        "kzg_lookup_multiplicities": (i, [vp, vp, sz, vp, sz, sz, sz, vp, vp, C.POINTER(sz)]),
        "kzg_lookup_multiplicities_device": (i, [vp, vp, sz, vp, sz, sz, sz, vp, vp, C.POINTER(sz)]),
        "kzg_lookup_multiplicities_cap": (i, [vp, vp, sz, vp, sz, sz, sz, vp, vp, C.POINTER(sz), C.c_uint]),
        "kzg_coset_extend": (i, [vp, vp, sz, sz, sz, C.c_uint, C.c_uint, vp]),
        "kzg_coset_extend_device": (i, [vp, vp, sz, sz, sz, C.c_uint, C.c_uint, vp]),
        "kzg_permutation_constraints_coset": (i, [vp, vp, vp, vp, sz, sz, sz, sz, vp, vp, vp, vp, vp, vp]),
        "kzg_permutation_constraints_coset_device": (i, [vp, vp, vp, vp, sz, sz, sz, sz, vp, vp, vp, vp, vp, vp]),
        "kzg_vanishing_quotient": (i, [vp, vp, sz, sz, i, vp]),
        "kzg_vanishing_quotient_device": (i, [vp, vp, sz, sz, i, vp]),
        "kzg_permutation_quotient": (i, [vp, vp, vp, vp, sz, sz, sz, vp, vp, vp, vp, vp, C.c_uint, vp, vp]),
        "kzg_circuit_create": (i, [vp, vp, vp, vp, vp, sz, sz, sz, vp, C.c_uint, vp, C.POINTER(vp)]),
        "kzg_circuit_destroy": (i, [vp, vp]),
        "kzg_circuit_create_lookup": (i, [vp, vp, vp, vp, vp, sz, sz, sz, vp, C.c_uint, vp, sz, sz, vp, vp, C.POINTER(vp)]),
        "kzg_circuit_lookup_columns": (i, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, C.POINTER(sz)]),
        "kzg_circuit_lookup_quotient": (i, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "kzg_circuit_lookup_prove": (i, [vp, vp, vp, vp, sz, vp, sz, vp, C.POINTER(sz)]),
        "kzg_circuit_lookup_prove_device": (i, [vp, vp, vp, vp, sz, vp, sz, vp, C.POINTER(sz)]),
        "kzg_circuit_lookup_blinded_sizes": (i, [sz, sz, C.c_uint, sz, C.POINTER(sz), C.POINTER(sz)]),
        "kzg_circuit_lookup_blinders": (i, [sz, C.c_uint, vp]),
        "kzg_circuit_lookup_quotient_blinded": (i, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "kzg_circuit_lookup_prove_blinded": (i, [vp, vp, vp, vp, sz, vp, sz, vp, vp, C.POINTER(sz)]),
        "kzg_circuit_lookup_prove_blinded_device": (i, [vp, vp, vp, vp, sz, vp, sz, vp, vp, C.POINTER(sz)]),
        "kzg_circuit_lookup_proof_size": (i, [sz, C.c_uint, sz, C.POINTER(sz)]),
        "kzg_circuit_lookup_proof_challenges": (i, [vp, sz, sz, C.c_uint, sz, vp, vp, sz, vp, sz, vp]),
        "kzg_circuit_lookup_verify_proof": (i, [vp, sz, sz, C.c_uint, sz, vp, vp, sz, vp, sz, vp, sz, vp, sz, C.POINTER(C.c_int)]),
        "kzg_circuit_create_custom": (i, [vp, vp, vp, vp, vp, sz, sz, sz, vp, C.c_uint, vp, sz, sz, vp, vp, C.POINTER(vp)]),
        "kzg_circuit_custom_gate": (i, [vp, vp, vp, sz, vp]),
        "kzg_circuit_custom_quotient": (i, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]),
        "kzg_circuit_custom_prove": (i, [vp, vp, vp, vp, sz, vp, sz, vp, vp]),
        "kzg_circuit_custom_prove_device": (i, [vp, vp, vp, vp, sz, vp, sz, vp, vp]),
        "kzg_circuit_custom_proof_challenges": (i, [vp, sz, sz, C.c_uint, sz, vp, vp, vp, sz, vp, sz, vp]),
        "kzg_circuit_custom_verify_proof": (i, [vp, sz, sz, C.c_uint, sz, vp, vp, vp, sz, vp, sz, vp, sz, vp, sz, C.POINTER(C.c_int)]),
        "kzg_circuit_custom_blinded_sizes": (i, [sz, sz, C.c_uint, sz, C.POINTER(sz), C.POINTER(sz)]),
        "kzg_circuit_verify_proofs_batch": (i, [vp, vp, sz, sz, C.c_uint, sz, vp, vp, vp, sz, sz, vp, sz, sz, vp, sz, C.POINTER(i),
                                                C.POINTER(sz)]),
        "kzg_circuit_verify_proofs_lincomb": (i, [vp, vp, sz, sz, C.c_uint, sz, vp, vp, vp, sz, sz, vp, sz, sz, vp, sz, vp, vp,
                                                  C.POINTER(i), C.POINTER(sz)]),
        "kzg_circuit_verify_proofs_lincomb_challenges": (i, [vp, vp, sz, sz, C.c_uint, sz, vp, vp, vp, sz, sz, vp, sz, sz, vp, sz, vp, vp, vp,
                                                             C.POINTER(i), C.POINTER(sz)]),
        "kzg_circuit_create_custom_next": (i, [vp, vp, vp, vp, vp, sz, sz, sz, vp, C.c_uint, vp, sz, sz, vp, vp, vp, C.POINTER(vp)]),
        "kzg_circuit_custom_next_gate": (i, [vp, vp, vp, sz, vp]),
        "kzg_circuit_custom_next_quotient": (i, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp]),
        "kzg_circuit_custom_next_prove": (i, [vp, vp, vp, vp, sz, vp, sz, vp, vp]),
        "kzg_circuit_custom_next_prove_device": (i, [vp, vp, vp, vp, sz, vp, sz, vp, vp]),
        "kzg_circuit_custom_next_proof_size": (i, [sz, C.c_uint, sz, C.POINTER(sz)]),
        "kzg_circuit_custom_next_proof_challenges": (i, [vp, sz, sz, C.c_uint, sz, vp, vp, vp, vp, sz, vp, sz, vp]),
        "kzg_circuit_custom_next_verify_proof": (i, [vp, sz, sz, C.c_uint, sz, vp, vp, vp, vp, sz, vp, sz, vp, sz, vp, sz,
                                                     C.POINTER(C.c_int)]),
        "kzg_circuit_quotient": (i, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]),
        "kzg_circuit_quotient_device": (i, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp]),
        "kzg_circuit_column_device": (i, [vp, vp, C.c_uint, C.c_uint, C.POINTER(vp), C.POINTER(sz)]),
        "kzg_circuit_open": (i, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "kzg_circuit_open_device": (i, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "kzg_circuit_linearise": (i, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "kzg_circuit_blinded_sizes": (i, [sz, sz, C.c_uint, C.POINTER(sz), C.POINTER(sz)]),
        "kzg_circuit_blinders": (i, [sz, C.c_uint, vp]),
        "kzg_blind_evaluations": (i, [vp, vp, sz, sz, sz, vp, sz, vp, sz]),
        "kzg_commit_evaluations_blinded": (i, [vp, vp, sz, sz, sz, vp, sz, vp]),
        "kzg_circuit_quotient_blinded": (i, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]),
        "kzg_circuit_quotient_blinded_device": (i, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]),
        "kzg_circuit_open_blinded": (i, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "kzg_circuit_open_blinded_device": (i, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "kzg_circuit_verify": (i, [vp, sz, sz, C.c_uint, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, sz,
                                   C.POINTER(C.c_int)]),
        "kzg_circuit_prove": (i, [vp, vp, vp, vp, sz, vp, sz, vp, vp]),
        "kzg_circuit_prove_device": (i, [vp, vp, vp, vp, sz, vp, sz, vp, vp]),
        "kzg_circuit_proof_size": (i, [sz, C.c_uint, C.POINTER(sz)]),
        "kzg_circuit_proof_challenges": (i, [vp, sz, sz, C.c_uint, vp, vp, sz, vp, sz, vp]),
        "kzg_circuit_verify_proof": (i, [vp, sz, sz, C.c_uint, vp, vp, sz, vp, sz, vp, sz, vp, sz, C.POINTER(C.c_int)]),
        "kzg_cells_and_proofs": (i, [vp, vp, sz, C.c_uint, C.c_uint, vp, vp]),
        "kzg_cells_and_proofs_evaluations": (i, [vp, vp, sz, C.c_uint, C.c_uint, vp, vp]),
        "kzg_quotient_cells": (i, [vp, vp, sz, C.c_uint, C.c_uint, sz, sz, vp, C.POINTER(sz)]),
        "kzg_cells_and_proofs_fk20": (i, [vp, vp, sz, sz, sz, C.c_uint, C.c_uint, vp, vp]),
        "kzg_fk20_prepare": (i, [vp, sz, C.c_uint]),
        "kzg_g1_dft": (i, [vp, vp, sz, i, vp]),
        "kzg_recover_cells_and_proofs": (i, [vp, sz, C.c_uint, C.c_uint, vp, sz, vp, sz, vp, vp, vp]),
        "kzg_verify_cells_batch": (i, [vp, vp, sz, vp, vp, vp, vp, sz, C.c_uint, C.c_uint, vp, sz, C.POINTER(i)]),
        "kzg_verify_cells_lincomb": (i, [vp, vp, sz, vp, vp, vp, vp, sz, C.c_uint, C.c_uint, vp, sz, vp, vp, vp, C.POINTER(i)]),
        "kzg_evaluate_evaluations_batch": (i, [vp, vp, sz, sz, sz, vp, vp]),
        "kzg_verify_openings_batch": (i, [vp, vp, sz, vp, vp, vp, vp, sz, vp, sz, C.POINTER(i)]),
        "kzg_verify_openings_lincomb": (i, [vp, vp, sz, vp, vp, vp, vp, sz, vp, sz, vp, vp, vp, C.POINTER(i)]),
        "kzg_verify_evaluations_batch": (i, [vp, vp, sz, sz, sz, vp, vp, vp, vp, sz, vp, C.POINTER(i)]),
        "kzg_verify_cells_batch_bytes": (i, [vp, vp, sz, vp, vp, vp, vp, sz, C.c_uint, C.c_uint, C.c_uint, vp, sz, C.POINTER(i)]),
        "kzg_verify_cells_lincomb_bytes": (i, [vp, vp, sz, vp, vp, vp, vp, sz, C.c_uint, C.c_uint, C.c_uint, vp, sz, vp, vp, vp,
                                               C.POINTER(i)]),
        "kzg_verify_openings_batch_bytes": (i, [vp, vp, sz, vp, vp, vp, vp, sz, vp, sz, C.POINTER(i)]),
        "kzg_verify_openings_lincomb_bytes": (i, [vp, vp, sz, vp, vp, vp, vp, sz, vp, sz, vp, vp, vp, C.POINTER(i)]),
        "kzg_verify_blobs_batch_bytes": (i, [vp, vp, sz, sz, sz, C.c_uint, vp, vp, vp, vp, sz, vp, C.POINTER(i)]),
        "kzg_g1_uncompress_batch": (i, [vp, vp, sz, i, vp, C.POINTER(sz)]),
        "kzg_fr_from_bytes_batch": (i, [vp, vp, sz, vp, C.POINTER(sz)]),
        "kzg_blobs_to_commitments_bytes": (i, [vp, vp, sz, sz, sz, C.c_uint, vp]),
        "kzg_blobs_to_cells_and_proofs_bytes": (i, [vp, vp, sz, sz, sz, C.c_uint, C.c_uint, C.c_uint, vp, vp, vp]),
        "kzg_recover_cells_and_proofs_bytes": (i, [vp, sz, C.c_uint, C.c_uint, C.c_uint, vp, sz, vp, sz, vp, vp]),
        "kzg_g1_compress_batch": (i, [vp, vp, sz, vp]),
        "kzg_fr_to_bytes_batch": (i, [vp, vp, sz, vp, C.POINTER(sz)]),
        "kzg_srs_update": (i, [vp, u8p, C.c_uint64]),
        "kzg_srs_verify": (i, [vp, vp, sz, C.c_uint, C.POINTER(i), C.POINTER(C.c_uint), C.POINTER(sz)]),
        "kzg_srs_verify_lincomb": (i, [vp, vp, vp, sz, vp, vp, C.POINTER(i)]),
        "kzg_g2_mul": (i, [vp, u8p, vp]),
        "kzg_srs_verify_update": (i, [vp, vp, vp, C.POINTER(i)]),
        "kzg_open_combined": (i, [vp, vp, sz, sz, sz, vp, vp, vp, vp]),
        "kzg_open_combined_submit": (i, [vp, i, vp, sz, sz, sz, vp, vp]),
        "kzg_wait_combined": (i, [vp, i, vp, vp]),
        "kzg_get_combine_ms": (i, [vp, i, C.POINTER(C.c_float)]),
        "kzg_combine_polys": (i, [vp, vp, sz, sz, sz, vp, vp]),
        "kzg_evaluate_batch_at": (i, [vp, vp, sz, sz, sz, vp, vp]),
        "kzg_combine_claims": (i, [vp, vp, sz, vp, vp, vp]),
        "kzg_verify_combined": (i, [vp, vp, sz, vp, vp, vp, vp, C.POINTER(i)]),
        "kzg_open_sets": (i, [vp, vp, sz, sz, sz, vp, vp, sz, vp, vp, vp, vp]),
        "kzg_open_sets_submit": (i, [vp, i, vp, sz, sz, sz, vp, vp, sz, vp, vp]),
        "kzg_wait_sets": (i, [vp, i, vp, vp]),
        "kzg_quotient_sets": (i, [vp, vp, sz, sz, sz, vp, vp, sz, vp, vp, vp, vp, C.POINTER(sz)]),
        "kzg_verify_sets": (i, [vp, sz, vp, vp, sz, vp, vp, vp, vp, vp, sz, vp, sz, C.POINTER(i)]),
        "kzg_ml_fold": (i, [vp, vp, sz, vp, vp]),
        "kzg_ml_evaluate": (i, [vp, vp, sz, vp, vp]),
        "kzg_ml_fold_device": (i, [vp, vp, sz, vp, vp, vp]),
        "kzg_ml_commit_folds_device": (i, [vp, vp, sz, vp]),
        "kzg_ml_evaluations_device": (i, [vp, vp, vp, sz, vp, vp]),
        "kzg_ml_open_device": (i, [vp, vp, vp, sz, vp, vp, vp]),
        "kzg_ml_open": (i, [vp, vp, sz, vp, vp, vp, vp, vp, vp, vp]),
        "kzg_ml_verify": (i, [vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, sz, C.POINTER(i)]),
        "kzg_sha256": (i, [vp, sz, vp]),
        "kzg_sha256_pieces": (i, [vp, sz, sz, i, vp]),
        "kzg_sha256_has_shani": (i, []),
        "kzg_blob_challenges_bytes": (i, [vp, sz, sz, sz, vp, vp]),
        "kzg_blobs_open_at_bytes": (i, [vp, vp, sz, sz, sz, C.c_uint, vp, vp, vp]),
        "kzg_blobs_to_blob_proofs_bytes": (i, [vp, vp, sz, sz, sz, C.c_uint, vp, vp, vp]),
        "kzg_verify_blob_proofs_batch_bytes": (i, [vp, vp, sz, sz, sz, C.c_uint, vp, vp, vp, sz, C.POINTER(i)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _LIB = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------
# Scalar: reference src/scalar.rs.  Value semantics on a canonical integer; `limbs()` is the
# blst_fr memory image (4 x u64, Montgomery) that crosses the C-ABI.
# ---------------------------------------------------------------------------------------------
class Scalar:
    __slots__ = ("v",)

    def __init__(self, v=0):
        self.v = int(v) % R_MODULUS

    @staticmethod
    def from_i128(a):  # src/scalar.rs:27-48: a > 0 -> a ; a <= 0 -> r - |a|
        a = int(a)
        if not -(1 << 127) <= a < (1 << 127):
            raise OverflowError("not an i128")
        return Scalar(a if a > 0 else R_MODULUS - (-a))

    @staticmethod
    def from_le_bytes(b):  # src/scalar.rs:54-61
        assert len(b) == 32
        return Scalar(int.from_bytes(bytes(b), "little"))

    @staticmethod
    def from_be_bytes(b):  # src/scalar.rs:66-73
        assert len(b) == 32
        return Scalar(int.from_bytes(bytes(b), "big"))

    @staticmethod
    def from_limbs(l):
        raw = sum(int(x) << (64 * i) for i, x in enumerate(l))
        return Scalar(raw * _FR_RINV)

    def to_le_bytes(self):  # src/scalar.rs:83-93
        return self.v.to_bytes(32, "little")

    def to_be_bytes(self):  # src/scalar.rs:96-106
        return self.v.to_bytes(32, "big")

    def limbs(self):
        m = self.v * _FR_R % R_MODULUS
        return np.array([(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)

    def mul(self, o):
        return Scalar(self.v * o.v)

    def add(self, o):
        return Scalar(self.v + o.v)

    def sub(self, o):
        return Scalar(self.v - o.v)

    def neg(self):
        return Scalar(-self.v)

    def pow(self, n):  # src/scalar.rs:122-187 (same value)
        return Scalar(pow(self.v, int(n), R_MODULUS))

    def is_zero(self):
        return self.v == 0

    def __eq__(self, o):
        return isinstance(o, Scalar) and self.v == o.v

    def __hash__(self):
        return hash(self.v)

    def __repr__(self):
        return "Scalar(%d)" % self.v

    def __str__(self):  # base-10 Display, src/scalar.rs:277-341
        return str(self.v)


def scalars_to_limbs(values):
    """ints (canonical, any sign) -> (n, 4) uint64 Montgomery blst_fr array."""
    out = np.empty((len(values), 4), dtype=np.uint64)
    mask = 0xFFFFFFFFFFFFFFFF
    for i, v in enumerate(values):
        m = (int(v) % R_MODULUS) * _FR_R % R_MODULUS
        out[i, 0] = m & mask
        out[i, 1] = (m >> 64) & mask
        out[i, 2] = (m >> 128) & mask
        out[i, 3] = m >> 192
    return out


def limbs_to_scalars(arr):
    arr = np.asarray(arr, dtype=np.uint64).reshape(-1, 4)
    out = []
    for row in arr:
        raw = int(row[0]) | (int(row[1]) << 64) | (int(row[2]) << 128) | (int(row[3]) << 192)
        out.append(raw * _FR_RINV % R_MODULUS)
    return out


# ---------------------------------------------------------------------------------------------
# G1Point: reference src/curves.rs:10-17 (a wrapped blst_p1).  Serialisation = 48 compressed bytes
# (src/curves.rs:99-110), which is also how two points are compared for parity.
# ---------------------------------------------------------------------------------------------
class G1Point:
    __slots__ = ("p1",)

    def __init__(self, p1):
        self.p1 = np.ascontiguousarray(p1, dtype=np.uint64).reshape(18)

    def compress(self):
        out = (C.c_ubyte * 48)()
        rc = load_library().kzg_g1_compress(_ptr(self.p1), C.cast(out, C.c_void_p))
        _check(rc)
        return bytes(out)

    @staticmethod
    def uncompress(data):  # Deserialize for G1Point, src/curves.rs:112-183
        out = np.zeros(18, dtype=np.uint64)
        _check(load_library().kzg_g1_uncompress(bytes(data), _ptr(out)))
        return G1Point(out)

    def is_infinity(self):
        return not self.p1[12:18].any()

    def add(self, other):  # src/curves.rs:79-85
        return G1Point.sum([self, other])

    @staticmethod
    def sum(points):
        arr = np.ascontiguousarray(np.stack([p.p1 for p in points]), dtype=np.uint64)
        out = np.zeros(18, dtype=np.uint64)
        _check(load_library().kzg_g1_sum(_ptr(arr), len(points), _ptr(out)))
        return G1Point(out)

    def __eq__(self, o):
        return isinstance(o, G1Point) and self.compress() == o.compress()

    def __repr__(self):
        return "G1Point(%s)" % self.compress().hex()


def _check(rc, ctx=None):
    if rc == KZG_OK:
        return
    lib = load_library()
    msg = lib.kzg_strerror(rc).decode()
    if rc == KZG_ERR_HIP and ctx is not None:
        msg += ": " + lib.kzg_last_error(ctx).decode()
    raise KzgError(rc, msg)


# ---------------------------------------------------------------------------------------------
# Engine: one context = one GPU with a resident SRS (no reference analogue; see kzg_mi355x.h).
# ---------------------------------------------------------------------------------------------
class Engine:
    def __init__(self, device=0, devices=None, replicate=False):
        """device: one HIP device.  devices=[d0, d1, ...]: one context over several devices (kzg_ctx_create_multi):
        the SRS is split by point range and commit / open shard transparently; a device may repeat (virtual slices).
        replicate=True (kzg_ctx_create_multi_ex, KZG_MULTI_REPLICATE_SRS): every device keeps the whole SRS and
        batches are split by polynomial, with nothing to exchange."""
        self._lib = load_library()
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int * len(devices))(*[int(d) for d in devices])
            if replicate:
                _check(self._lib.kzg_ctx_create_multi_ex(arr, len(devices), KZG_MULTI_REPLICATE_SRS, C.byref(h)))
            else:
                _check(self._lib.kzg_ctx_create_multi(arr, len(devices), C.byref(h)))
            device = int(devices[0])
        else:
            _check(self._lib.kzg_ctx_create(int(device), C.byref(h)))
        self._h = h
        self.device = device

    def num_devices(self):
        return int(self._lib.kzg_num_devices(self._h))

    def rccl_exchanges(self):
        return int(self._lib.kzg_rccl_exchanges(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.kzg_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- SRS --
    def srs_load(self, p1_array, stride=None):
        """p1_array: (n, k>=18) uint64 rows starting with a blst_p1 (the g1 of a SetupArtifact)."""
        a = np.ascontiguousarray(p1_array, dtype=np.uint64)
        n = a.shape[0]
        stride = a.strides[0] if stride is None else stride
        _check(self._lib.kzg_srs_load_g1(self._h, _ptr(a), stride, n), self._h)

    def srs_load_affine(self, xy_array):
        """(n, 12) uint64: x, y as blst_fp (Montgomery); (0, 0) = infinity"""
        a = np.ascontiguousarray(xy_array, dtype=np.uint64).reshape(-1, 12)
        _check(self._lib.kzg_srs_load_affine(self._h, _ptr(a), a.shape[0]), self._h)

    def srs_load_compressed(self, data):
        """n x 48 bytes (ZCash encoding); raises KzgError with .bad_index on a malformed point"""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        assert buf.size % 48 == 0
        bad = C.c_size_t(0)
        rc = self._lib.kzg_srs_load_compressed(self._h, _ptr(buf), buf.size // 48, C.byref(bad))
        if rc != KZG_OK:
            e = KzgError(rc, self._lib.kzg_strerror(rc).decode() + ": " + self._lib.kzg_last_error(self._h).decode())
            e.bad_index = None if bad.value == C.c_size_t(-1).value else int(bad.value)
            raise e

    def srs_save(self, path):
        _check(self._lib.kzg_srs_save(self._h, os.fsencode(path)), self._h)

    def srs_load_file(self, path):
        _check(self._lib.kzg_srs_load_file(self._h, os.fsencode(path)), self._h)

    def srs_generate(self, secret_be, n, first=0):
        _check(self._lib.kzg_srs_generate_g1(self._h, bytes(secret_be), first, n), self._h)

    def srs_read(self, index, count):
        out = np.zeros((count, 18), dtype=np.uint64)
        _check(self._lib.kzg_srs_read_g1(self._h, index, count, _ptr(out)), self._h)
        return out

    def srs_len(self):
        return int(self._lib.kzg_srs_len(self._h))

    # -- powers-of-tau ceremonies --
    def _error(self, rc):
        return KzgError(rc, self._lib.kzg_strerror(rc).decode() + ": " + self._lib.kzg_last_error(self._h).decode())

    def srs_update(self, tau_be, first=0):
        """kzg_srs_update: SRS[i] <- [tau^(first + i)] SRS[i] on the device; tau: 32 bytes big-endian, reduced mod r.
        Raises KzgError(KZG_ERR_INVALID_ARG) for tau = 0 mod r and leaves the SRS as it was"""
        assert len(tau_be) == 32
        rc = self._lib.kzg_srs_update(self._h, bytes(tau_be), int(first))
        if rc != KZG_OK:
            raise self._error(rc)

    def srs_verify(self, setup_g2, require_generator=True):
        """kzg_srs_verify: is the resident SRS [s^i]G1 for the s of setup_g2 = ([1]G2, [s]G2) (blst_p2 rows)?  Returns
        (valid, reason, bad_index): reason one of the KZG_SRS_* codes, bad_index the point it names or None"""
        g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
        assert g2.shape[0] >= 2
        ok, reason, bad = C.c_int(0), C.c_uint(0), C.c_size_t(0)
        rc = self._lib.kzg_srs_verify(self._h, _ptr(g2), 288, KZG_SRS_FIRST_IS_GENERATOR if require_generator else 0,
                                      C.byref(ok), C.byref(reason), C.byref(bad))
        if rc != KZG_OK:
            raise self._error(rc)
        return bool(ok.value), int(reason.value), (None if bad.value == C.c_size_t(-1).value else int(bad.value))

    def srs_verify_lincomb(self, weights, setup_g2):
        """the test hook kzg_srs_verify_lincomb: weights: srs_len() - 1 Scalars (or blst_fr rows).  Returns (A, B, valid):
        A = sum rho_i SRS[i], B = sum rho_i SRS[i + 1] as G1Points and the pairing's answer"""
        g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
        w = (np.ascontiguousarray(weights, dtype=np.uint64).reshape(-1, 4) if isinstance(weights, np.ndarray)
             else _scalar_rows(weights))
        a = np.zeros(18, dtype=np.uint64)
        b = np.zeros(18, dtype=np.uint64)
        ok = C.c_int(0)
        rc = self._lib.kzg_srs_verify_lincomb(self._h, _ptr(w), _ptr(g2), 288, _ptr(a), _ptr(b), C.byref(ok))
        if rc != KZG_OK:
            raise self._error(rc)
        return G1Point(a), G1Point(b), bool(ok.value)

    def msm_config(self):
        c, w, nb, rec = C.c_int(), C.c_int(), C.c_size_t(), C.c_int()
        _check(self._lib.kzg_msm_config(self._h, C.byref(c), C.byref(w), C.byref(nb), C.byref(rec)))
        return {"recoding": "naf" if rec.value == 1 else "windows", "digit_bits": c.value,
                "table_levels": w.value, "buckets": nb.value}

    # -- hot path, host buffers --
    def commit_limbs(self, coeffs):
        a = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(18, dtype=np.uint64)
        _check(self._lib.kzg_commit(self._h, _ptr(a), a.shape[0], _ptr(out)), self._h)
        return G1Point(out)

    def commit_le_bytes(self, scalars_le):
        a = np.ascontiguousarray(np.frombuffer(bytes(scalars_le), dtype=np.uint8))
        out = np.zeros(18, dtype=np.uint64)
        _check(self._lib.kzg_commit_le_bytes(self._h, _ptr(a), a.size // 32, _ptr(out)), self._h)
        return G1Point(out)

    def open_limbs(self, coeffs, z, y):
        a = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        zl, yl = z.limbs(), y.limbs()
        out = np.zeros(18, dtype=np.uint64)
        _check(self._lib.kzg_open(self._h, _ptr(a), a.shape[0], _ptr(zl), _ptr(yl), _ptr(out)), self._h)
        return G1Point(out)

    def quotient_limbs(self, coeffs, z, y):
        a = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        zl, yl = z.limbs(), y.limbs()
        q = np.zeros((max(a.shape[0], 1), 4), dtype=np.uint64)
        qn = C.c_size_t(0)
        _check(self._lib.kzg_quotient(self._h, _ptr(a), a.shape[0], _ptr(zl), _ptr(yl), _ptr(q), C.byref(qn)), self._h)
        return q[: qn.value].copy()

    def evaluate_limbs(self, coeffs, z):
        a = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        zl = z.limbs()
        out = np.zeros(4, dtype=np.uint64)
        _check(self._lib.kzg_evaluate(self._h, _ptr(a), a.shape[0], _ptr(zl), _ptr(out)), self._h)
        return Scalar.from_limbs(out)

    # -- multiproofs: one proof for P at k points (zs, ys: sequences of Scalar) --
    def open_points_limbs(self, coeffs, zs, ys):
        a = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        zl, yl = _scalar_rows(zs), _scalar_rows(ys)
        out = np.zeros(18, dtype=np.uint64)
        _check(self._lib.kzg_open_points(self._h, _ptr(a), a.shape[0], _ptr(zl), _ptr(yl), len(zs), _ptr(out)), self._h)
        return G1Point(out)

    def open_points_submit(self, slot, dptr, n, zs, ys):
        zl, yl = _scalar_rows(zs), _scalar_rows(ys)
        _check(self._lib.kzg_open_points_submit(self._h, slot, C.c_void_p(dptr), n, _ptr(zl), _ptr(yl), len(zs)), self._h)

    def quotient_points_limbs(self, coeffs, zs, ys):
        a = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        zl, yl = _scalar_rows(zs), _scalar_rows(ys)
        q = np.zeros((max(a.shape[0] - len(zs), 1), 4), dtype=np.uint64)
        qn = C.c_size_t(0)
        _check(self._lib.kzg_quotient_points(self._h, _ptr(a), a.shape[0], _ptr(zl), _ptr(yl), len(zs), _ptr(q), C.byref(qn)),
               self._h)
        return q[: qn.value].copy()

    def evaluate_points_limbs(self, coeffs, zs):
        a = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        zl = _scalar_rows(zs)
        out = np.zeros((max(len(zs), 1), 4), dtype=np.uint64)
        _check(self._lib.kzg_evaluate_points(self._h, _ptr(a), a.shape[0], _ptr(zl), len(zs), _ptr(out)), self._h)
        return [Scalar.from_limbs(out[i]) for i in range(len(zs))]

    # -- combined openings: t polynomials at one point, one proof for F = sum gamma^i P_i (z, gamma: Scalar) --
    @staticmethod
    def _combine_block(polys, stride):
        """list of (n, 4) arrays or one (t, n, 4) array -> (flat uint64 block, n, t, stride): polynomial i at row i * stride"""
        a = Engine._stack(polys)
        t, n = a.shape[0], a.shape[1]
        stride = n if stride is None else stride
        if stride != n:
            assert stride >= n or t == 1
            block = np.zeros((t, max(stride, n), 4), dtype=np.uint64)
            block[:, :n] = a
            a = block
        return np.ascontiguousarray(a), n, t, stride

    def open_combined_limbs(self, polys, z, gamma, stride=None):
        """kzg_open_combined: returns ([P_i(z)], proof) for equally long polynomials in host memory"""
        flat, n, t, stride = self._combine_block(polys, stride)
        zl, gl = z.limbs(), gamma.limbs()
        ys = np.zeros((t, 4), dtype=np.uint64)
        out = np.zeros(18, dtype=np.uint64)
        _check(self._lib.kzg_open_combined(self._h, _ptr(flat), n, t, stride, _ptr(zl), _ptr(gl), _ptr(ys), _ptr(out)), self._h)
        return [Scalar.from_limbs(ys[i]) for i in range(t)], G1Point(out)

    def open_combined_submit(self, slot, dptr, n, t, z, gamma, stride=None):
        zl, gl = z.limbs(), gamma.limbs()
        _check(self._lib.kzg_open_combined_submit(self._h, slot, C.c_void_p(dptr), n, t, n if stride is None else stride,
                                                  _ptr(zl), _ptr(gl)), self._h)

    def wait_combined(self, slot, t):
        ys = np.zeros((max(t, 1), 4), dtype=np.uint64)
        out = np.zeros(18, dtype=np.uint64)
        _check(self._lib.kzg_wait_combined(self._h, slot, _ptr(ys), _ptr(out)), self._h)
        return [Scalar.from_limbs(ys[i]) for i in range(t)], G1Point(out)

    def combine_ms(self, slot):
        """with set_timing(True): the duration of the slot's last combination pass, in ms"""
        ms = C.c_float(0)
        _check(self._lib.kzg_get_combine_ms(self._h, slot, C.byref(ms)), self._h)
        return float(ms.value)

    def combine_polys_limbs(self, polys, gamma, stride=None):
        """kzg_combine_polys: the coefficients of F = sum gamma^i P_i as an (n, 4) array of blst_fr images"""
        flat, n, t, stride = self._combine_block(polys, stride)
        gl = gamma.limbs()
        out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        _check(self._lib.kzg_combine_polys(self._h, _ptr(flat), n, t, stride, _ptr(gl), _ptr(out)), self._h)
        return out[:n].copy()

    def evaluate_batch_at_limbs(self, polys, z, stride=None):
        """kzg_evaluate_batch_at: [P_i(z)]"""
        flat, n, t, stride = self._combine_block(polys, stride)
        zl = z.limbs()
        ys = np.zeros((t, 4), dtype=np.uint64)
        _check(self._lib.kzg_evaluate_batch_at(self._h, _ptr(flat), n, t, stride, _ptr(zl), _ptr(ys)), self._h)
        return [Scalar.from_limbs(ys[i]) for i in range(t)]

    # -- openings at several point sets: polynomial i on sets[set_of[i]], one proof (sets: lists of Scalar; gamma: Scalar) --
    def open_sets_limbs(self, polys, set_of, sets, gamma, stride=None):
        """kzg_open_sets: returns (ys, proof), ys[i] the values of polynomial i on its set, in the set's point order"""
        flat, n, t, stride = self._combine_block(polys, stride)
        so, sl, zl = _sets_arrays(set_of, sets)
        assert len(set_of) == t
        ys = np.zeros((_sets_value_count(set_of, sets), 4), dtype=np.uint64)
        out = np.zeros(18, dtype=np.uint64)
        _check(self._lib.kzg_open_sets(self._h, _ptr(flat), n, t, stride, _ptr(so), _ptr(sl), len(sets), _ptr(zl),
                                       _ptr(gamma.limbs()), _ptr(ys), _ptr(out)), self._h)
        return _sets_split_values(ys, set_of, sets), G1Point(out)

    def open_sets_submit(self, slot, dptr, n, t, set_of, sets, gamma, stride=None):
        so, sl, zl = _sets_arrays(set_of, sets)
        assert len(set_of) == t
        _check(self._lib.kzg_open_sets_submit(self._h, slot, C.c_void_p(dptr), n, t, n if stride is None else stride, _ptr(so),
                                              _ptr(sl), len(sets), _ptr(zl), _ptr(gamma.limbs())), self._h)

    def wait_sets(self, slot, set_of, sets):
        """kzg_wait_sets: (ys, proof) of the slot's job; set_of, sets as submitted (they give the shape of ys)"""
        ys = np.zeros((_sets_value_count(set_of, sets), 4), dtype=np.uint64)
        out = np.zeros(18, dtype=np.uint64)
        _check(self._lib.kzg_wait_sets(self._h, slot, _ptr(ys), _ptr(out)), self._h)
        return _sets_split_values(ys, set_of, sets), G1Point(out)

    def quotient_sets_limbs(self, polys, set_of, sets, gamma, stride=None):
        """kzg_quotient_sets: (ys, h) with h the quotient's coefficients without trailing zeros, an (n', 4) array of images"""
        flat, n, t, stride = self._combine_block(polys, stride)
        so, sl, zl = _sets_arrays(set_of, sets)
        assert len(set_of) == t
        ys = np.zeros((_sets_value_count(set_of, sets), 4), dtype=np.uint64)
        h = np.zeros((max(n - 1, 1), 4), dtype=np.uint64)
        hn = C.c_size_t(0)
        _check(self._lib.kzg_quotient_sets(self._h, _ptr(flat), n, t, stride, _ptr(so), _ptr(sl), len(sets), _ptr(zl),
                                           _ptr(gamma.limbs()), _ptr(ys), _ptr(h), C.byref(hn)), self._h)
        return _sets_split_values(ys, set_of, sets), h[: hn.value].copy()

    # -- every cell of the domain of N = 2^log_domain points and its multiproof (cells of 2^log_cell points) --
    def _cells(self, fn, values, log_domain, log_cell):
        a = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        cells = np.zeros((1 << log_domain, 4), dtype=np.uint64)
        proofs = np.zeros((max(1 << max(log_domain - log_cell, 0), 1), 18), dtype=np.uint64)
        _check(fn(self._h, _ptr(a), a.shape[0], log_domain, log_cell, _ptr(cells), _ptr(proofs)), self._h)
        return cells, [G1Point(p) for p in proofs[: 1 << max(log_domain - log_cell, 0)]]

    def cells_and_proofs_limbs(self, coeffs, log_domain, log_cell):
        """(cells, proofs): cells[j l + i] = P(w_N^(j + (N/l) i)) as an (N, 4) array, proofs[j] the multiproof of cell j"""
        return self._cells(self._lib.kzg_cells_and_proofs, coeffs, log_domain, log_cell)

    def cells_and_proofs_from_evaluations_limbs(self, evals, log_domain, log_cell):
        """the same for P given by its values over the len(evals)-point domain (a power of two <= N)"""
        return self._cells(self._lib.kzg_cells_and_proofs_evaluations, evals, log_domain, log_cell)

    def cells_and_proofs_fk20(self, coeffs, log_domain, log_cell, cells=True):
        """FK20 for a batch: coeffs is a (batch, n, 4) array (or one (n, 4) polynomial).  Returns (cells, proofs):
        cells a (batch, N, 4) array (None when cells=False), proofs[b][j] the multiproof of cell j of polynomial b --
        each equal to what cells_and_proofs_limbs returns for that polynomial"""
        a = np.ascontiguousarray(coeffs, dtype=np.uint64)
        if a.ndim != 3:
            a = a.reshape(1, a.size // 4, 4)
        batch, n = a.shape[0], a.shape[1]
        M = 1 << max(log_domain - log_cell, 0)
        out_cells = np.zeros((batch, 1 << log_domain, 4), dtype=np.uint64) if cells else None
        proofs = np.zeros((max(batch, 1), M, 18), dtype=np.uint64)
        _check(self._lib.kzg_cells_and_proofs_fk20(self._h, _ptr(a), n, batch, n, log_domain, log_cell,
                                                   _ptr(out_cells) if cells else None, _ptr(proofs)), self._h)
        return out_cells, [[G1Point(p) for p in proofs[b]] for b in range(batch)]

    def recover_cells_and_proofs(self, n, log_domain, log_cell, cell_ids, cells, coeffs=True, cells_out=True, proofs=True):
        """Rebuilds polynomials of n coefficients from k of their N/l cells: cell_ids lists the k distinct received cells (any
        order, shared by the batch), cells is a (batch, k, l, 4) array (or (k, l, 4) for one polynomial), row t holding cell
        cell_ids[t].  Returns (coeffs, cells, proofs) shaped as cells_and_proofs_fk20 returns them -- coeffs (batch, n, 4),
        cells (batch, N, 4), proofs[b][j] -- each None when not requested"""
        ids = np.ascontiguousarray(cell_ids, dtype=np.uint32).reshape(-1)
        a = np.ascontiguousarray(cells, dtype=np.uint64)
        if a.ndim != 4:
            a = a.reshape(1, len(ids), 1 << log_cell, 4)
        batch = a.shape[0]
        M = 1 << max(log_domain - log_cell, 0)
        out_c = np.zeros((batch, n, 4), dtype=np.uint64) if coeffs else None
        out_v = np.zeros((batch, 1 << log_domain, 4), dtype=np.uint64) if cells_out else None
        out_p = np.zeros((max(batch, 1), M, 18), dtype=np.uint64) if proofs else None
        opt = lambda x: _ptr(x) if x is not None else None  # noqa: E731
        _check(self._lib.kzg_recover_cells_and_proofs(self._h, n, log_domain, log_cell, _ptr(ids), len(ids), _ptr(a), batch,
                                                      opt(out_c), opt(out_v), opt(out_p)), self._h)
        return out_c, out_v, ([[G1Point(p) for p in out_p[b]] for b in range(batch)] if proofs else None)

    def _verify_cells_args(self, commitments, commitment_idx, cell_ids, cells, proofs, log_cell, setup_g2):
        rows = lambda pts, w: np.ascontiguousarray(  # noqa: E731
            np.stack([p.p1 if isinstance(p, G1Point) else np.asarray(p, dtype=np.uint64) for p in pts])
            if len(pts) else np.zeros((0, w), dtype=np.uint64), dtype=np.uint64).reshape(-1, w)
        com = rows(list(commitments), 18)
        prf = rows(list(proofs), 18)
        idx = np.ascontiguousarray(commitment_idx, dtype=np.uint32).reshape(-1)
        ids = np.ascontiguousarray(cell_ids, dtype=np.uint32).reshape(-1)
        k = len(ids)
        vals = np.ascontiguousarray(cells, dtype=np.uint64).reshape(k, 1 << log_cell, 4) if k else np.zeros((1, 4), np.uint64)
        g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
        assert len(idx) == k and prf.shape[0] == k, "one commitment index, cell id, value row and proof per record"
        keep = (com, prf, idx, ids, vals, g2)
        return keep, (_ptr(com) if com.size else None, com.shape[0], _ptr(idx) if k else None, _ptr(ids) if k else None,
                      _ptr(vals) if k else None, _ptr(prf) if k else None, k)

    def verify_cells_batch(self, commitments, commitment_idx, cell_ids, cells, proofs, log_domain, log_cell, setup_g2):
        """kzg_verify_cells_batch: checks k cell records at once with one pairing (random weights).  commitments: G1Points
        (or blst_p1 rows); record t claims that commitments[commitment_idx[t]] opens to cells[t] (l x 4 limbs) on cell
        cell_ids[t] with proofs[t]; setup_g2: blst_p2 rows [s^j]G2 for j <= l.  Returns True when every record is valid"""
        keep, a = self._verify_cells_args(commitments, commitment_idx, cell_ids, cells, proofs, log_cell, setup_g2)
        ok = C.c_int(0)
        _check(self._lib.kzg_verify_cells_batch(self._h, *a, log_domain, log_cell, _ptr(keep[5]), 288, C.byref(ok)), self._h)
        return bool(ok.value)

    def verify_cells_lincomb(self, commitments, commitment_idx, cell_ids, cells, proofs, log_domain, log_cell, setup_g2, weights):
        """the test hook kzg_verify_cells_lincomb: the same check with the given weights (k blst_fr rows, or Scalars).
        Returns (lhs, rhs, valid): the two G1 sides as G1Points and the pairing's answer"""
        keep, a = self._verify_cells_args(commitments, commitment_idx, cell_ids, cells, proofs, log_cell, setup_g2)
        w = (np.ascontiguousarray(weights, dtype=np.uint64).reshape(-1, 4) if isinstance(weights, np.ndarray)
             else _scalar_rows(weights))
        lhs = np.zeros(18, dtype=np.uint64)
        rhs = np.zeros(18, dtype=np.uint64)
        ok = C.c_int(0)
        _check(self._lib.kzg_verify_cells_lincomb(self._h, *a, log_domain, log_cell, _ptr(keep[5]), 288, _ptr(w), _ptr(lhs),
                                                  _ptr(rhs), C.byref(ok)), self._h)
        return G1Point(lhs), G1Point(rhs), bool(ok.value)

    # -- openings at arbitrary points --
    @staticmethod
    def _fr_rows(values):
        """Scalars or blst_fr rows -> (k, 4) uint64"""
        if isinstance(values, np.ndarray):
            return np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        return _scalar_rows(list(values)) if len(values) else np.zeros((0, 4), dtype=np.uint64)

    @staticmethod
    def _p1_rows(pts):
        pts = list(pts)
        if not pts:
            return np.zeros((0, 18), dtype=np.uint64)
        return np.ascontiguousarray(np.stack([p.p1 if isinstance(p, G1Point) else np.asarray(p, dtype=np.uint64) for p in pts]),
                                    dtype=np.uint64).reshape(-1, 18)

    def evaluate_evaluations_batch(self, evals, zs):
        """kzg_evaluate_evaluations_batch: evals a (batch, n, 4) array (or one (n, 4) polynomial) of values over the n-domain,
        zs one point per polynomial (Scalars or blst_fr rows).  Returns the P_b(z_b) as a list of Scalars"""
        a = np.ascontiguousarray(evals, dtype=np.uint64)
        if a.ndim != 3:
            a = a.reshape(1, a.size // 4, 4)
        batch, n = a.shape[0], a.shape[1]
        zl = self._fr_rows(zs)
        assert zl.shape[0] == batch, "one point per polynomial"
        out = np.zeros((max(batch, 1), 4), dtype=np.uint64)
        _check(self._lib.kzg_evaluate_evaluations_batch(self._h, _ptr(a), n, batch, n, _ptr(zl) if batch else None, _ptr(out)),
               self._h)
        return [Scalar.from_limbs(out[b]) for b in range(batch)]

    def _verify_openings_args(self, commitments, commitment_idx, zs, ys, proofs, setup_g2):
        com, prf = self._p1_rows(commitments), self._p1_rows(proofs)
        idx = np.ascontiguousarray(commitment_idx, dtype=np.uint32).reshape(-1)
        zl, yl = self._fr_rows(zs), self._fr_rows(ys)
        k = len(idx)
        g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
        assert zl.shape[0] == k and yl.shape[0] == k and prf.shape[0] == k, "one index, point, value and proof per record"
        keep = (com, prf, idx, zl, yl, g2)
        return keep, (_ptr(com) if com.size else None, com.shape[0], _ptr(idx) if k else None, _ptr(zl) if k else None,
                      _ptr(yl) if k else None, _ptr(prf) if k else None, k, _ptr(g2), 288)

    def verify_openings_batch(self, commitments, commitment_idx, zs, ys, proofs, setup_g2):
        """kzg_verify_openings_batch: checks k openings at arbitrary points with one pairing (random weights).  Record t
        claims that commitments[commitment_idx[t]] opens to ys[t] at zs[t] with proofs[t]; setup_g2: blst_p2 rows [1]G2,
        [s]G2.  Returns True when every record is valid"""
        keep, a = self._verify_openings_args(commitments, commitment_idx, zs, ys, proofs, setup_g2)
        ok = C.c_int(0)
        _check(self._lib.kzg_verify_openings_batch(self._h, *a, C.byref(ok)), self._h)
        return bool(ok.value)

    def verify_openings_lincomb(self, commitments, commitment_idx, zs, ys, proofs, setup_g2, weights):
        """the test hook kzg_verify_openings_lincomb: the same check with the given weights (k blst_fr rows, or Scalars).
        Returns (lhs, rhs, valid): the two G1 sides as G1Points and the pairing's answer"""
        keep, a = self._verify_openings_args(commitments, commitment_idx, zs, ys, proofs, setup_g2)
        w = self._fr_rows(weights)
        if not w.shape[0]:
            w = np.zeros((1, 4), dtype=np.uint64)
        lhs = np.zeros(18, dtype=np.uint64)
        rhs = np.zeros(18, dtype=np.uint64)
        ok = C.c_int(0)
        _check(self._lib.kzg_verify_openings_lincomb(self._h, *a, _ptr(w), _ptr(lhs), _ptr(rhs), C.byref(ok)), self._h)
        return G1Point(lhs), G1Point(rhs), bool(ok.value)

    def verify_evaluations_batch(self, evals, commitments, zs, proofs, setup_g2, want_ys=True):
        """kzg_verify_evaluations_batch: polynomial b of evals ((batch, n, 4) values over the n-domain) is claimed to have
        commitments[b] and the opening proofs[b] at zs[b].  Returns (valid, ys): ys the values P_b(z_b) the device computed
        (None when want_ys is False)"""
        a = np.ascontiguousarray(evals, dtype=np.uint64)
        if a.ndim != 3:
            a = a.reshape(1, a.size // 4, 4)
        batch, n = a.shape[0], a.shape[1]
        com, prf, zl = self._p1_rows(commitments), self._p1_rows(proofs), self._fr_rows(zs)
        g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
        assert com.shape[0] == batch and prf.shape[0] == batch and zl.shape[0] == batch
        out = np.zeros((max(batch, 1), 4), dtype=np.uint64) if want_ys else None
        ok = C.c_int(0)
        opt = lambda x: _ptr(x) if x is not None and x.size else None  # noqa: E731
        _check(self._lib.kzg_verify_evaluations_batch(self._h, _ptr(a), n, batch, n, opt(com), opt(zl), opt(prf), _ptr(g2), 288,
                                                      opt(out), C.byref(ok)), self._h)
        return bool(ok.value), ([Scalar.from_limbs(out[b]) for b in range(batch)] if want_ys else None)

    # -- the verifiers on inputs as they travel --
    @staticmethod
    def _wire(data, width):
        """bytes, or anything numpy reads as uint8 -> a contiguous (count, width) uint8 array"""
        a = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else \
            np.ascontiguousarray(data, dtype=np.uint8)
        assert a.size % width == 0, "a whole number of %d-byte strings" % width
        return np.ascontiguousarray(a).reshape(-1, width)

    def g1_uncompress_batch(self, data, check_subgroup=False):
        """kzg_g1_uncompress_batch: n x 48 bytes of compressed points -> (n, 18) blst_p1 rows, decoded on the device.  A
        point that does not decode (or, with check_subgroup, lies outside G1) raises KzgError; its index is in .bad_index"""
        a = self._wire(data, 48)
        out = np.zeros((max(a.shape[0], 1), 18), dtype=np.uint64)
        bad = C.c_size_t(0)
        rc = self._lib.kzg_g1_uncompress_batch(self._h, _ptr(a) if a.size else None, a.shape[0], 1 if check_subgroup else 0,
                                               _ptr(out), C.byref(bad))
        self._check_bad(rc, bad)
        return out[:a.shape[0]]

    def fr_from_bytes_batch(self, data):
        """kzg_fr_from_bytes_batch: n x 32 big-endian bytes -> (n, 4) blst_fr rows; a value not below r raises KzgError with
        its index in .bad_index"""
        a = self._wire(data, 32)
        out = np.zeros((max(a.shape[0], 1), 4), dtype=np.uint64)
        bad = C.c_size_t(0)
        rc = self._lib.kzg_fr_from_bytes_batch(self._h, _ptr(a) if a.size else None, a.shape[0], _ptr(out), C.byref(bad))
        self._check_bad(rc, bad)
        return out[:a.shape[0]]

    def _check_bad(self, rc, bad):
        try:
            _check(rc, self._h)
        except KzgError as e:
            e.bad_index = None if bad.value == C.c_size_t(-1).value else bad.value
            raise

    def _verify_cells_bytes_args(self, commitments48, commitment_idx, cell_ids, cells_be, proofs48, log_cell, setup_g2):
        com, prf = self._wire(commitments48, 48), self._wire(proofs48, 48)
        idx = np.ascontiguousarray(commitment_idx, dtype=np.uint32).reshape(-1)
        ids = np.ascontiguousarray(cell_ids, dtype=np.uint32).reshape(-1)
        k = len(ids)
        vals = self._wire(cells_be, 32)
        g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
        assert len(idx) == k and prf.shape[0] == k and vals.shape[0] == k << log_cell, \
            "one commitment index, cell id, row of l values and proof per record"
        keep = (com, prf, idx, ids, vals, g2)
        return keep, (_ptr(com) if com.size else None, com.shape[0], _ptr(idx) if k else None, _ptr(ids) if k else None,
                      _ptr(vals) if k else None, _ptr(prf) if k else None, k)

    def verify_cells_batch_bytes(self, commitments48, commitment_idx, cell_ids, cells_be, proofs48, log_domain, log_cell,
                                 setup_g2, order=KZG_ORDER_NATURAL):
        """kzg_verify_cells_batch_bytes: verify_cells_batch on the wire forms -- commitments48 / proofs48: 48-byte compressed
        points, cells_be: k x l x 32 big-endian bytes (bytes or uint8 arrays); order KZG_ORDER_BIT_REVERSED: cell ids and
        values in the sampling specs' bit-reversed order"""
        keep, a = self._verify_cells_bytes_args(commitments48, commitment_idx, cell_ids, cells_be, proofs48, log_cell, setup_g2)
        ok = C.c_int(0)
        _check(self._lib.kzg_verify_cells_batch_bytes(self._h, *a, log_domain, log_cell, order, _ptr(keep[5]), 288,
                                                      C.byref(ok)), self._h)
        return bool(ok.value)

    def verify_cells_lincomb_bytes(self, commitments48, commitment_idx, cell_ids, cells_be, proofs48, log_domain, log_cell,
                                   setup_g2, weights, order=KZG_ORDER_NATURAL):
        """the test hook kzg_verify_cells_lincomb_bytes; returns (lhs, rhs, valid) as verify_cells_lincomb"""
        keep, a = self._verify_cells_bytes_args(commitments48, commitment_idx, cell_ids, cells_be, proofs48, log_cell, setup_g2)
        w = self._fr_rows(weights)
        if not w.shape[0]:
            w = np.zeros((1, 4), dtype=np.uint64)
        lhs = np.zeros(18, dtype=np.uint64)
        rhs = np.zeros(18, dtype=np.uint64)
        ok = C.c_int(0)
        _check(self._lib.kzg_verify_cells_lincomb_bytes(self._h, *a, log_domain, log_cell, order, _ptr(keep[5]), 288, _ptr(w),
                                                        _ptr(lhs), _ptr(rhs), C.byref(ok)), self._h)
        return G1Point(lhs), G1Point(rhs), bool(ok.value)

    def _verify_openings_bytes_args(self, commitments48, commitment_idx, zs_be, ys_be, proofs48, setup_g2):
        com, prf = self._wire(commitments48, 48), self._wire(proofs48, 48)
        idx = np.ascontiguousarray(commitment_idx, dtype=np.uint32).reshape(-1)
        zl, yl = self._wire(zs_be, 32), self._wire(ys_be, 32)
        k = len(idx)
        g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
        assert zl.shape[0] == k and yl.shape[0] == k and prf.shape[0] == k, "one index, point, value and proof per record"
        keep = (com, prf, idx, zl, yl, g2)
        return keep, (_ptr(com) if com.size else None, com.shape[0], _ptr(idx) if k else None, _ptr(zl) if k else None,
                      _ptr(yl) if k else None, _ptr(prf) if k else None, k, _ptr(g2), 288)

    def verify_openings_batch_bytes(self, commitments48, commitment_idx, zs_be, ys_be, proofs48, setup_g2):
        """kzg_verify_openings_batch_bytes: verify_openings_batch on 48-byte compressed points and 32-byte big-endian scalars"""
        keep, a = self._verify_openings_bytes_args(commitments48, commitment_idx, zs_be, ys_be, proofs48, setup_g2)
        ok = C.c_int(0)
        _check(self._lib.kzg_verify_openings_batch_bytes(self._h, *a, C.byref(ok)), self._h)
        return bool(ok.value)

    def verify_openings_lincomb_bytes(self, commitments48, commitment_idx, zs_be, ys_be, proofs48, setup_g2, weights):
        """the test hook kzg_verify_openings_lincomb_bytes; returns (lhs, rhs, valid) as verify_openings_lincomb"""
        keep, a = self._verify_openings_bytes_args(commitments48, commitment_idx, zs_be, ys_be, proofs48, setup_g2)
        w = self._fr_rows(weights)
        if not w.shape[0]:
            w = np.zeros((1, 4), dtype=np.uint64)
        lhs = np.zeros(18, dtype=np.uint64)
        rhs = np.zeros(18, dtype=np.uint64)
        ok = C.c_int(0)
        _check(self._lib.kzg_verify_openings_lincomb_bytes(self._h, *a, _ptr(w), _ptr(lhs), _ptr(rhs), C.byref(ok)), self._h)
        return G1Point(lhs), G1Point(rhs), bool(ok.value)

    def _circuit_verify_batch_args(self, key, n, log_ext, shifts, public_inputs, proofs, setup_g2, exponents, n_public):
        t = len(shifts)
        ex = None if exponents is None else np.ascontiguousarray(exponents, dtype=np.uint8).reshape(-1, t)
        g = 0 if ex is None else ex.shape[0]
        assert len(key) == 2 * t + 2 + g
        rows = np.ascontiguousarray(np.stack([c.p1 for c in key]), dtype=np.uint64)
        proofs = [bytes(p) for p in proofs]
        count = len(proofs)
        proof_len = len(proofs[0]) if count else circuit_proof_size(t, log_ext)
        assert all(len(p) == proof_len for p in proofs), "proofs of one length"
        buf = np.frombuffer(b"".join(proofs), dtype=np.uint8) if count else None
        if public_inputs is None:
            pub, stride, n_public = None, 0, 0
        elif isinstance(public_inputs, np.ndarray):  # (count, pi_stride, 4) blst_fr rows, the first n_public of a row are read
            pub = np.ascontiguousarray(public_inputs, dtype=np.uint64)
            pub = pub.reshape(count, -1, 4) if count else np.zeros((0, n_public or 0, 4), dtype=np.uint64)
            stride = pub.shape[1]
            n_public = stride if n_public is None else n_public
        else:  # one list of Scalars per proof
            assert len(public_inputs) == count and len({len(p) for p in public_inputs}) <= 1
            n_public = len(public_inputs[0]) if count else 0
            stride = n_public
            pub = np.stack([_scalar_rows(list(p)) for p in public_inputs]) if n_public else None
        g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
        assert g2.shape[0] >= 3
        ks = _scalar_rows(shifts)
        keep = (rows, ex, ks, pub, buf, g2)
        opt = lambda x: _ptr(x) if x is not None and x.size else None  # noqa: E731
        return keep, count, (_ptr(rows), n, t, log_ext, g, opt(ex), _ptr(ks), opt(pub), n_public, stride, opt(buf), proof_len, count,
                             _ptr(g2), 288)

    def circuit_verify_proofs_batch(self, key, n, log_ext, shifts, public_inputs, proofs, setup_g2, exponents=None, n_public=None):
        """kzg_circuit_verify_proofs_batch: checks many proofs (a list of proof bytes) of the one key with one pairing.
        public_inputs: None, one list of Scalars per proof, or a (count, pi_stride, 4) array of which the first n_public
        values per proof are read; exponents: the (g, t) bytes of a custom circuit, whose key has 2 t + 2 + g commitments;
        setup_g2: blst_p2 rows [1]G2, [s]G2, [s^2]G2.  Returns (ok, bad_index): bad_index the least proof that does not decode
        or has a point outside G1, None when there is none (the pairing alone does not locate a proof)"""
        keep, count, a = self._circuit_verify_batch_args(key, n, log_ext, shifts, public_inputs, proofs, setup_g2, exponents, n_public)
        ok, bad = C.c_int(0), C.c_size_t(0)
        _check(self._lib.kzg_circuit_verify_proofs_batch(self._h, *a, C.byref(ok), C.byref(bad)), self._h)
        return bool(ok.value), (None if bad.value == C.c_size_t(-1).value else int(bad.value))

    def circuit_verify_proofs_lincomb(self, key, n, log_ext, shifts, public_inputs, proofs, setup_g2, weights, exponents=None,
                                      n_public=None, challenges=None):
        """the test hook kzg_circuit_verify_proofs_lincomb: the same check with the given weights (one blst_fr row or Scalar per
        proof).  Returns (ok, bad_index, (P0, P1, P2)): the three G1 sums as G1Points.  challenges (5 Scalars per proof: beta,
        gamma, alpha, zeta, v): kzg_circuit_verify_proofs_lincomb_challenges, which takes them in the place of the hashed ones"""
        keep, count, a = self._circuit_verify_batch_args(key, n, log_ext, shifts, public_inputs, proofs, setup_g2, exponents, n_public)
        w = self._fr_rows(weights)
        assert w.shape[0] == count, "one weight per proof"
        if not count:
            w = np.zeros((1, 4), dtype=np.uint64)
        out = np.zeros((3, 18), dtype=np.uint64)
        ok, bad = C.c_int(0), C.c_size_t(0)
        if challenges is None:
            _check(self._lib.kzg_circuit_verify_proofs_lincomb(self._h, *a, _ptr(w), _ptr(out), C.byref(ok), C.byref(bad)), self._h)
        else:
            ch = self._fr_rows([c for five in challenges for c in five])
            assert ch.shape[0] == 5 * count, "five challenges per proof"
            _check(self._lib.kzg_circuit_verify_proofs_lincomb_challenges(self._h, *a, _ptr(w), _ptr(ch) if count else None, _ptr(out),
                                                                          C.byref(ok), C.byref(bad)), self._h)
        return bool(ok.value), (None if bad.value == C.c_size_t(-1).value else int(bad.value)), tuple(G1Point(out[i].copy()) for i in range(3))

    def verify_blobs_batch_bytes(self, blobs_be, n, commitments48, zs_be, proofs48, setup_g2, order=KZG_ORDER_NATURAL,
                                 want_ys=True):
        """kzg_verify_blobs_batch_bytes: verify_evaluations_batch for blobs as they travel -- blobs_be: batch x n x 32
        big-endian bytes.  Returns (valid, ys_be): the values P_b(z_b) as batch x 32 big-endian bytes (None when want_ys is
        False)"""
        a = self._wire(blobs_be, 32)
        assert n and a.shape[0] % n == 0, "whole blobs of n values"
        batch = a.shape[0] // n
        com, prf, zl = self._wire(commitments48, 48), self._wire(proofs48, 48), self._wire(zs_be, 32)
        g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
        assert com.shape[0] == batch and prf.shape[0] == batch and zl.shape[0] == batch
        out = np.zeros((max(batch, 1), 32), dtype=np.uint8) if want_ys else None
        ok = C.c_int(0)
        opt = lambda x: _ptr(x) if x is not None and x.size else None  # noqa: E731
        _check(self._lib.kzg_verify_blobs_batch_bytes(self._h, opt(a), n, batch, n, order, opt(com), opt(zl), opt(prf), _ptr(g2),
                                                      288, opt(out), C.byref(ok)), self._h)
        return bool(ok.value), (out[:batch].tobytes() if want_ys else None)

    # -- the producing side on blobs as they travel --
    def g1_compress_batch(self, points):
        """kzg_g1_compress_batch: n blst_p1 rows (an (n, 18) array, or G1Points; any Z) -> n x 48 bytes, normalised and encoded
        on the device"""
        a = self._p1_rows(points) if not isinstance(points, np.ndarray) else np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 18)
        n = a.shape[0]
        out = np.zeros((max(n, 1), 48), dtype=np.uint8)
        _check(self._lib.kzg_g1_compress_batch(self._h, _ptr(a) if n else None, n, _ptr(out)), self._h)
        return out[:n].tobytes()

    def fr_to_bytes_batch(self, values):
        """kzg_fr_to_bytes_batch: (n, 4) blst_fr rows -> n x 32 big-endian bytes; a row not below r raises KzgError with its
        index in .bad_index"""
        a = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        n = a.shape[0]
        out = np.zeros((max(n, 1), 32), dtype=np.uint8)
        bad = C.c_size_t(0)
        rc = self._lib.kzg_fr_to_bytes_batch(self._h, _ptr(a) if n else None, n, _ptr(out), C.byref(bad))
        self._check_bad(rc, bad)
        return out[:n].tobytes()

    def _blobs(self, blobs_be, n, stride):
        a = self._wire(blobs_be, 32)
        stride = n if stride is None else stride
        if not (n and stride >= n and a.shape[0] % stride == 0):  # (not an assert: the C side trusts these lengths)
            raise ValueError("whole blobs of n values, `stride` values apart")
        return a, a.shape[0] // stride, stride

    def blobs_to_commitments_bytes(self, blobs_be, n, order=KZG_ORDER_NATURAL, stride=None):
        """kzg_blobs_to_commitments_bytes: batch x stride x 32 big-endian bytes (bytes or a uint8 array; the first n values of
        every stride are the blob) -> batch x 48 bytes of compressed commitments"""
        a, batch, stride = self._blobs(blobs_be, n, stride)
        out = np.zeros((max(batch, 1), 48), dtype=np.uint8)
        _check(self._lib.kzg_blobs_to_commitments_bytes(self._h, _ptr(a) if a.size else None, n, batch, stride, order, _ptr(out)),
               self._h)
        return out[:batch].tobytes()

    def blobs_to_cells_and_proofs_bytes(self, blobs_be, n, log_domain, log_cell, order=KZG_ORDER_NATURAL, commitments=True,
                                        cells=True, stride=None):
        """kzg_blobs_to_cells_and_proofs_bytes: returns (commitments48, cells_be, proofs48) as bytes -- batch x 48, batch x N x
        32 and batch x (N / l) x 48 of them; commitments48 / cells_be are None when not requested"""
        a, batch, stride = self._blobs(blobs_be, n, stride)
        N = 1 << log_domain
        M = 1 << max(log_domain - log_cell, 0)
        out_c = np.zeros((max(batch, 1), 48), dtype=np.uint8) if commitments else None
        out_v = np.zeros((max(batch, 1), N * 32), dtype=np.uint8) if cells else None
        out_p = np.zeros((max(batch, 1), M * 48), dtype=np.uint8)
        opt = lambda x: _ptr(x) if x is not None else None  # noqa: E731
        _check(self._lib.kzg_blobs_to_cells_and_proofs_bytes(self._h, _ptr(a) if a.size else None, n, batch, stride, log_domain,
                                                             log_cell, order, opt(out_c), opt(out_v), _ptr(out_p)), self._h)
        return (out_c[:batch].tobytes() if commitments else None, out_v[:batch].tobytes() if cells else None,
                out_p[:batch].tobytes())

    def recover_cells_and_proofs_bytes(self, n, log_domain, log_cell, cell_ids, cells_be, order=KZG_ORDER_NATURAL, cells_out=True,
                                       proofs=True):
        """kzg_recover_cells_and_proofs_bytes: cells_be is batch x k x l x 32 big-endian bytes, row t of a polynomial holding
        cell cell_ids[t] (ids and the values inside a cell in the order asked).  Returns (cells_be, proofs48) as
        blobs_to_cells_and_proofs_bytes returns them, each None when not requested"""
        ids = np.ascontiguousarray(cell_ids, dtype=np.uint32).reshape(-1)
        a = self._wire(cells_be, 32)
        per = len(ids) << log_cell
        if not (per and a.shape[0] % per == 0):
            raise ValueError("k cells of l values per polynomial")
        batch = a.shape[0] // per
        N = 1 << log_domain
        M = 1 << max(log_domain - log_cell, 0)
        out_v = np.zeros((max(batch, 1), N * 32), dtype=np.uint8) if cells_out else None
        out_p = np.zeros((max(batch, 1), M * 48), dtype=np.uint8) if proofs else None
        opt = lambda x: _ptr(x) if x is not None else None  # noqa: E731
        _check(self._lib.kzg_recover_cells_and_proofs_bytes(self._h, n, log_domain, log_cell, order, _ptr(ids), len(ids),
                                                            _ptr(a) if a.size else None, batch, opt(out_v), opt(out_p)), self._h)
        return (out_v[:batch].tobytes() if cells_out else None, out_p[:batch].tobytes() if proofs else None)

    # -- blob proofs and their Fiat-Shamir challenges --
    def blobs_open_at_bytes(self, blobs_be, n, zs_be, order=KZG_ORDER_NATURAL, stride=None):
        """kzg_blobs_open_at_bytes: blobs as blobs_to_commitments_bytes takes them and one point per blob (batch x 32
        big-endian bytes) -> (ys_be, proofs48): the values P_b(z_b), batch x 32 bytes, and the proofs of those openings,
        batch x 48 bytes"""
        a, batch, stride = self._blobs(blobs_be, n, stride)
        zl = self._wire(zs_be, 32)
        if zl.shape[0] != batch:
            raise ValueError("one point per blob")
        ys = np.zeros((max(batch, 1), 32), dtype=np.uint8)
        out = np.zeros((max(batch, 1), 48), dtype=np.uint8)
        _check(self._lib.kzg_blobs_open_at_bytes(self._h, _ptr(a) if a.size else None, n, batch, stride, order,
                                                 _ptr(zl) if zl.size else None, _ptr(ys), _ptr(out)), self._h)
        return ys[:batch].tobytes(), out[:batch].tobytes()

    def blobs_to_blob_proofs_bytes(self, blobs_be, n, commitments48=None, order=KZG_ORDER_NATURAL, stride=None):
        """kzg_blobs_to_blob_proofs_bytes: the proof of every blob at its Fiat-Shamir challenge.  commitments48: batch x 48
        bytes hashed as given, or None to have them computed.  Returns (commitments48, proofs48) as bytes"""
        a, batch, stride = self._blobs(blobs_be, n, stride)
        com = None
        if commitments48 is not None:
            com = self._wire(commitments48, 48)
            if com.shape[0] != batch:
                raise ValueError("one commitment per blob")
        out_c = np.zeros((max(batch, 1), 48), dtype=np.uint8)
        out_p = np.zeros((max(batch, 1), 48), dtype=np.uint8)
        _check(self._lib.kzg_blobs_to_blob_proofs_bytes(self._h, _ptr(a) if a.size else None, n, batch, stride, order,
                                                        _ptr(com) if com is not None and com.size else None, _ptr(out_c),
                                                        _ptr(out_p)), self._h)
        return out_c[:batch].tobytes(), out_p[:batch].tobytes()

    def verify_blob_proofs_batch_bytes(self, blobs_be, n, commitments48, proofs48, setup_g2, order=KZG_ORDER_NATURAL, stride=None):
        """kzg_verify_blob_proofs_batch_bytes: verify_blobs_batch_bytes at the challenges derived from each blob and its
        commitment; returns the verdict"""
        a, batch, stride = self._blobs(blobs_be, n, stride)
        com, prf = self._wire(commitments48, 48), self._wire(proofs48, 48)
        g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
        if com.shape[0] != batch or prf.shape[0] != batch:
            raise ValueError("one commitment and one proof per blob")
        ok = C.c_int(0)
        opt = lambda x: _ptr(x) if x is not None and x.size else None  # noqa: E731
        _check(self._lib.kzg_verify_blob_proofs_batch_bytes(self._h, opt(a), n, batch, stride, order, opt(com), opt(prf), _ptr(g2),
                                                            288, C.byref(ok)), self._h)
        return bool(ok.value)

    def fk20_prepare(self, n, log_cell):
        """builds the SRS-side FK20 transforms for polynomials of n coefficients and cells of 2^log_cell points now"""
        _check(self._lib.kzg_fk20_prepare(self._h, n, log_cell), self._h)

    def g1_dft(self, points, inverse=False):
        """DFT of m = 2^k G1 points (G1Point or blst_p1 rows) over w_m: out[j] = sum_i [w_m^(i j)] points[i];
        inverse: the inverse transform, 1/m included"""
        a = np.ascontiguousarray([p.p1 if isinstance(p, G1Point) else p for p in points], dtype=np.uint64).reshape(-1, 18)
        out = np.zeros_like(a)
        _check(self._lib.kzg_g1_dft(self._h, _ptr(a), a.shape[0], 1 if inverse else 0, _ptr(out)), self._h)
        return [G1Point(p) for p in out]

    def quotient_cells_limbs(self, coeffs, log_domain, log_cell, first_cell=0, count=None):
        """quotients of cells [first_cell, first_cell + count): an array (count, n' - l, 4)"""
        a = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        n, l = a.shape[0], 1 << log_cell
        if count is None:
            count = (1 << log_domain >> log_cell) - first_cell
        q = np.zeros((max(count, 1), max(n - l, 1), 4), dtype=np.uint64)
        qn = C.c_size_t(0)
        _check(self._lib.kzg_quotient_cells(self._h, _ptr(a), n, log_domain, log_cell, first_cell, count, _ptr(q), C.byref(qn)),
               self._h)
        return q[:count, : qn.value].copy()

    # -- polynomials in evaluation form over the domain {w^i} of size n = 2^k (natural order, see domain_root) --
    def _ntt(self, values, inverse):
        a = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros_like(a)
        _check(self._lib.kzg_ntt(self._h, _ptr(a), a.shape[0], 1 if inverse else 0, _ptr(out)), self._h)
        return out

    def ntt_limbs(self, coeffs):
        """coefficients -> evaluations: out[i] = P(w^i)"""
        return self._ntt(coeffs, False)

    def intt_limbs(self, evals):
        """evaluations -> coefficients (the interpolation, 1/n included)"""
        return self._ntt(evals, True)

    def ntt_device(self, d_in, d_out, n, inverse=False):
        _check(self._lib.kzg_ntt_device(self._h, C.c_void_p(d_in), C.c_void_p(d_out), n, 1 if inverse else 0), self._h)

    def ntt_batch_limbs(self, columns, n, inverse=False, out=None):
        """kzg_ntt of every column in one call.  columns: an array (batch, in_stride, 4) whose column b holds its n values
        first (in_stride >= n; the rows after them are not read).  out: an array (batch, out_stride, 4) written in place
        (only the first n rows of each column; out may be `columns` itself), or None for a new (batch, n, 4) array."""
        a = np.ascontiguousarray(columns, dtype=np.uint64)
        assert a.ndim == 3 and a.shape[2] == 4, "columns: (batch, in_stride, 4)"
        if out is None:
            out = np.zeros((a.shape[0], n, 4), dtype=np.uint64)
        assert out.dtype == np.uint64 and out.flags.c_contiguous and out.ndim == 3 and out.shape[0] == a.shape[0] and out.shape[2] == 4
        _check(self._lib.kzg_ntt_batch(self._h, _ptr(a), n, a.shape[0], a.shape[1], 1 if inverse else 0, _ptr(out), out.shape[1]),
               self._h)
        return out

    def ntt_batch_rounds(self, n, batch):
        """kzg_ntt_batch_rounds: the rounds a batched transform of `batch` columns of n values takes on this context"""
        out = C.c_size_t(0)
        _check(self._lib.kzg_ntt_batch_rounds(self._h, n, batch, C.byref(out)), self._h)
        return out.value

    def ntt_batch_device(self, d_in, n, batch, in_stride, d_out, out_stride, inverse=False):
        """the same on device buffers: column b at d_in + 32 b in_stride bytes, to d_out + 32 b out_stride bytes"""
        _check(self._lib.kzg_ntt_batch_device(self._h, C.c_void_p(d_in), n, batch, in_stride, C.c_void_p(d_out), out_stride,
                                              1 if inverse else 0), self._h)

    def commit_evaluations_limbs(self, evals):
        a = np.ascontiguousarray(evals, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(18, dtype=np.uint64)
        _check(self._lib.kzg_commit_evaluations(self._h, _ptr(a), a.shape[0], _ptr(out)), self._h)
        return G1Point(out)

    def commit_evaluations_submit(self, slot, dptr, n):
        _check(self._lib.kzg_commit_evaluations_submit(self._h, slot, C.c_void_p(dptr), n), self._h)

    def open_evaluations_limbs(self, evals, z, y):
        a = np.ascontiguousarray(evals, dtype=np.uint64).reshape(-1, 4)
        zl, yl = z.limbs(), y.limbs()
        out = np.zeros(18, dtype=np.uint64)
        _check(self._lib.kzg_open_evaluations(self._h, _ptr(a), a.shape[0], _ptr(zl), _ptr(yl), _ptr(out)), self._h)
        return G1Point(out)

    # -- the Lagrange basis of the n-domain: commitments and openings from values with no inverse NTT --
    def lagrange_prepare(self, log_n):
        """kzg_lagrange_prepare: builds (or replaces) the basis L_i = [l_i(s)] G1 of the 2^log_n-domain"""
        _check(self._lib.kzg_lagrange_prepare(self._h, int(log_n)), self._h)

    def lagrange_len(self):
        return int(self._lib.kzg_lagrange_len(self._h))

    def lagrange_read(self, index, count):
        out = np.zeros((count, 18), dtype=np.uint64)
        _check(self._lib.kzg_lagrange_read_g1(self._h, index, count, _ptr(out)), self._h)
        return out

    def _lagrange_bytes(self, fn, data, order, *more):
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        assert buf.size % 48 == 0
        bad = C.c_size_t(0)
        rc = fn(self._h, _ptr(buf), buf.size // 48, int(order), *more, C.byref(bad))
        if rc != KZG_OK:
            e = self._error(rc)
            e.bad_index = None if bad.value == C.c_size_t(-1).value else int(bad.value)
            raise e

    def lagrange_load_compressed(self, data, order=KZG_ORDER_NATURAL, check=True):
        """kzg_lagrange_load_compressed: adopts the basis given as n x 48 bytes.  Returns whether it was adopted: False when
        check found it inconsistent with the resident SRS.  Raises KzgError with .bad_index for a malformed point"""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        assert buf.size % 48 == 0
        bad, ok = C.c_size_t(0), C.c_int(0)
        rc = self._lib.kzg_lagrange_load_compressed(self._h, _ptr(buf), buf.size // 48, int(order), 1 if check else 0,
                                                    C.byref(bad), C.byref(ok))
        if rc != KZG_OK:
            e = self._error(rc)
            e.bad_index = None if bad.value == C.c_size_t(-1).value else int(bad.value)
            raise e
        return bool(ok.value) if check else True

    def srs_load_lagrange_compressed(self, data, order=KZG_ORDER_NATURAL):
        """kzg_srs_load_lagrange_compressed: a setup that exists only in Lagrange form (n x 48 bytes) becomes the SRS and
        its Lagrange basis"""
        self._lagrange_bytes(self._lib.kzg_srs_load_lagrange_compressed, data, order)

    def commit_lagrange_limbs(self, evals):
        a = np.ascontiguousarray(evals, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(18, dtype=np.uint64)
        _check(self._lib.kzg_commit_lagrange(self._h, _ptr(a), a.shape[0], _ptr(out)), self._h)
        return G1Point(out)

    def commit_lagrange_submit(self, slot, dptr, n):
        _check(self._lib.kzg_commit_lagrange_submit(self._h, slot, C.c_void_p(dptr), n), self._h)

    def commit_lagrange_batch(self, evals, n=None):
        """kzg_commit_lagrange_batch: evals a (batch, stride, 4) array (or a list of equally long (stride, 4) arrays) whose
        first n values per row are the polynomial's (n=None: all of them)"""
        flat = self._stack(evals)
        b, rows = flat.shape[0], flat.shape[1]
        n = rows if n is None else int(n)
        out = np.zeros((b, 18), dtype=np.uint64)
        _check(self._lib.kzg_commit_lagrange_batch(self._h, _ptr(flat), n, b, rows, _ptr(out)), self._h)
        return [G1Point(out[i]) for i in range(b)]

    def open_lagrange_limbs(self, evals, z, y):
        a = np.ascontiguousarray(evals, dtype=np.uint64).reshape(-1, 4)
        zl, yl = z.limbs(), y.limbs()
        out = np.zeros(18, dtype=np.uint64)
        _check(self._lib.kzg_open_lagrange(self._h, _ptr(a), a.shape[0], _ptr(zl), _ptr(yl), _ptr(out)), self._h)
        return G1Point(out)

    def open_lagrange_submit(self, slot, dptr, n, z, y):
        zl, yl = z.limbs(), y.limbs()
        _check(self._lib.kzg_open_lagrange_submit(self._h, slot, C.c_void_p(dptr), n, _ptr(zl), _ptr(yl)), self._h)

    def quotient_lagrange_limbs(self, evals, z, y):
        """kzg_quotient_lagrange: the n values of (P - y) / (X - z) over the domain"""
        a = np.ascontiguousarray(evals, dtype=np.uint64).reshape(-1, 4)
        zl, yl = z.limbs(), y.limbs()
        out = np.zeros_like(a)
        _check(self._lib.kzg_quotient_lagrange(self._h, _ptr(a), a.shape[0], _ptr(zl), _ptr(yl), _ptr(out)), self._h)
        return out

    # -- grand products: z_0 = 1, z_(i+1) = z_i A_i / B_i with one inversion per call --
    @staticmethod
    def _columns(cols, n):
        """(t, stride, 4) array (or a list of (stride, 4) arrays) -> the flat array, t, stride, n"""
        a = np.ascontiguousarray(cols, dtype=np.uint64)
        a = a.reshape(a.shape[0], -1, 4)
        return a, a.shape[0], a.shape[1], a.shape[1] if n is None else int(n)

    def _gp_status(self, rc, bad):
        if rc != KZG_OK:
            e = self._error(rc)
            e.bad_index = None if bad.value == C.c_size_t(-1).value else int(bad.value)
            raise e

    def grand_product_limbs(self, nums, dens, n=None):
        """kzg_grand_product: nums, dens (t, stride, 4) arrays whose first n rows per column count (n=None: all of them).
        Returns (z, last): z an (n, 4) array, last a (4,) array.  A zero denominator raises KzgError with .bad_index"""
        a, t, stride, n = self._columns(nums, n)
        b = np.ascontiguousarray(dens, dtype=np.uint64).reshape(t, stride, 4)
        z, last, bad = np.zeros((n, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64), C.c_size_t(0)
        self._gp_status(self._lib.kzg_grand_product(self._h, _ptr(a), _ptr(b), n, t, stride, _ptr(z), _ptr(last), C.byref(bad)), bad)
        return z, last

    def grand_product_device(self, d_nums, d_dens, n, t, d_out_z, stride=None):
        """kzg_grand_product_device on kzg_dev_alloc buffers: z lands in d_out_z, returns last"""
        last, bad = np.zeros(4, dtype=np.uint64), C.c_size_t(0)
        self._gp_status(self._lib.kzg_grand_product_device(self._h, C.c_void_p(d_nums), C.c_void_p(d_dens), n, t,
                                                           n if stride is None else stride, C.c_void_p(d_out_z), _ptr(last),
                                                           C.byref(bad)), bad)
        return last

    @staticmethod
    def _perm_scalars(shifts, beta, gamma, t):
        sh = np.ascontiguousarray([k.limbs() for k in shifts], dtype=np.uint64).reshape(-1, 4)
        assert sh.shape[0] == t, "one coset shift per column"
        return sh, beta.limbs(), gamma.limbs()

    def permutation_product_limbs(self, wires, sigmas, shifts, beta, gamma, n=None):
        """kzg_permutation_product: wires, sigmas (t, stride, 4) arrays, shifts t Scalars, beta and gamma Scalars -> (z, last)"""
        a, t, stride, n = self._columns(wires, n)
        b = np.ascontiguousarray(sigmas, dtype=np.uint64).reshape(t, stride, 4)
        sh, bl, gl = self._perm_scalars(shifts, beta, gamma, t)
        z, last, bad = np.zeros((n, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64), C.c_size_t(0)
        self._gp_status(self._lib.kzg_permutation_product(self._h, _ptr(a), _ptr(b), n, t, stride, _ptr(sh), _ptr(bl), _ptr(gl),
                                                          _ptr(z), _ptr(last), C.byref(bad)), bad)
        return z, last

    def permutation_product_device(self, d_wires, d_sigmas, n, t, shifts, beta, gamma, d_out_z, stride=None):
        sh, bl, gl = self._perm_scalars(shifts, beta, gamma, t)
        last, bad = np.zeros(4, dtype=np.uint64), C.c_size_t(0)
        self._gp_status(self._lib.kzg_permutation_product_device(self._h, C.c_void_p(d_wires), C.c_void_p(d_sigmas), n, t,
                                                                 n if stride is None else stride, _ptr(sh), _ptr(bl), _ptr(gl),
                                                                 C.c_void_p(d_out_z), _ptr(last), C.byref(bad)), bad)
        return last

    def permutation_commit(self, wires, sigmas, shifts, beta, gamma, n=None, want_z=True):
        """kzg_permutation_commit: z and its commitment over the Lagrange basis in one call -> (G1Point, z or None, last)"""
        a, t, stride, n = self._columns(wires, n)
        b = np.ascontiguousarray(sigmas, dtype=np.uint64).reshape(t, stride, 4)
        sh, bl, gl = self._perm_scalars(shifts, beta, gamma, t)
        z = np.zeros((n, 4), dtype=np.uint64) if want_z else None
        last, out, bad = np.zeros(4, dtype=np.uint64), np.zeros(18, dtype=np.uint64), C.c_size_t(0)
        self._gp_status(self._lib.kzg_permutation_commit(self._h, _ptr(a), _ptr(b), n, t, stride, _ptr(sh), _ptr(bl), _ptr(gl),
                                                         _ptr(z) if want_z else None, _ptr(last), _ptr(out), C.byref(bad)), bad)
        return G1Point(out), z, last

    # -- log-derivative lookup arguments: running sums, a batch inverse, multiplicities --
    def logderivative_sum_limbs(self, nums, dens, n=None):
        """kzg_logderivative_sum: nums (or None: every numerator is one), dens (t, stride, 4) arrays whose first n rows per column
        count (n=None: all).  Returns (phi, last): phi an (n, 4) array, last a (4,) array.  A zero denominator raises KzgError with
        .bad_index"""
        b, t, stride, n = self._columns(dens, n)
        a = None if nums is None else np.ascontiguousarray(nums, dtype=np.uint64).reshape(t, stride, 4)
        phi, last, bad = np.zeros((n, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64), C.c_size_t(0)
        self._gp_status(self._lib.kzg_logderivative_sum(self._h, None if a is None else _ptr(a), _ptr(b), n, t, stride, _ptr(phi),
                                                        _ptr(last), C.byref(bad)), bad)
        return phi, last

    def logderivative_sum_device(self, d_nums, d_dens, n, t, d_out_phi, stride=None):
        """kzg_logderivative_sum_device on kzg_dev_alloc buffers (d_nums None: numerators one): phi lands in d_out_phi, returns last"""
        last, bad = np.zeros(4, dtype=np.uint64), C.c_size_t(0)
        self._gp_status(self._lib.kzg_logderivative_sum_device(self._h, None if d_nums is None else C.c_void_p(d_nums), C.c_void_p(d_dens),
                                                               n, t, n if stride is None else stride, C.c_void_p(d_out_phi), _ptr(last),
                                                               C.byref(bad)), bad)
        return last

    def lookup_sum_limbs(self, lookups, table, mult, beta, n=None):
        """kzg_lookup_sum: lookups a (k, stride, 4) array, table and mult (n, 4) arrays, beta a Scalar -> (phi, last)"""
        f, k, stride, n = self._columns(lookups, n)
        tb = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1, 4)
        m = np.ascontiguousarray(mult, dtype=np.uint64).reshape(-1, 4)
        assert tb.shape[0] >= n and m.shape[0] >= n, "the table and its multiplicities have n rows"
        bl = beta.limbs()
        phi, last, bad = np.zeros((n, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64), C.c_size_t(0)
        self._gp_status(self._lib.kzg_lookup_sum(self._h, _ptr(f), n, k, stride, _ptr(tb), _ptr(m), _ptr(bl), _ptr(phi), _ptr(last),
                                                 C.byref(bad)), bad)
        return phi, last

    def lookup_sum_device(self, d_lookups, n, k, d_table, d_mult, beta, d_out_phi, stride=None):
        bl = beta.limbs()
        last, bad = np.zeros(4, dtype=np.uint64), C.c_size_t(0)
        self._gp_status(self._lib.kzg_lookup_sum_device(self._h, C.c_void_p(d_lookups), n, k, n if stride is None else stride,
                                                        C.c_void_p(d_table), C.c_void_p(d_mult), _ptr(bl), C.c_void_p(d_out_phi),
                                                        _ptr(last), C.byref(bad)), bad)
        return last

    def lookup_commit(self, lookups, table, mult, beta, n=None, want_phi=True):
        """kzg_lookup_commit: phi and its commitment over the Lagrange basis in one call -> (G1Point, phi or None, last)"""
        f, k, stride, n = self._columns(lookups, n)
        tb = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1, 4)
        m = np.ascontiguousarray(mult, dtype=np.uint64).reshape(-1, 4)
        assert tb.shape[0] >= n and m.shape[0] >= n, "the table and its multiplicities have n rows"
        bl = beta.limbs()
        phi = np.zeros((n, 4), dtype=np.uint64) if want_phi else None
        last, out, bad = np.zeros(4, dtype=np.uint64), np.zeros(18, dtype=np.uint64), C.c_size_t(0)
        self._gp_status(self._lib.kzg_lookup_commit(self._h, _ptr(f), n, k, stride, _ptr(tb), _ptr(m), _ptr(bl),
                                                    _ptr(phi) if want_phi else None, _ptr(last), _ptr(out), C.byref(bad)), bad)
        return G1Point(out), phi, last

    def batch_inverse_limbs(self, vals):
        """kzg_batch_inverse: vals an (n, 4) array -> the (n, 4) array of inverses.  A zero raises KzgError with .bad_index"""
        v = np.ascontiguousarray(vals, dtype=np.uint64).reshape(-1, 4)
        out, bad = np.zeros_like(v), C.c_size_t(0)
        self._gp_status(self._lib.kzg_batch_inverse(self._h, _ptr(v), v.shape[0], _ptr(out), C.byref(bad)), bad)
        return out

    def batch_inverse_device(self, d_vals, n, d_out):
        bad = C.c_size_t(0)
        self._gp_status(self._lib.kzg_batch_inverse_device(self._h, C.c_void_p(d_vals), n, C.c_void_p(d_out), C.byref(bad)), bad)

    def lookup_multiplicities(self, table, lookups, n=None, want_rows=True, log_capacity=None):
        """kzg_lookup_multiplicities: table an (n_table, 4) array, lookups a (k, stride, 4) array -> (mult (n_table, 4), rows (k, n)
        uint32 or None).  A looked-up value in no table row raises KzgError with .bad_index, the least such row.  log_capacity: the
        test hook kzg_lookup_multiplicities_cap"""
        tb = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1, 4)
        f, k, stride, n = self._columns(lookups, n)
        mult, bad = np.zeros_like(tb), C.c_size_t(0)
        rows = np.zeros((k, n), dtype=np.uint32) if want_rows else None
        args = (self._h, _ptr(tb), tb.shape[0], _ptr(f), n, k, stride, _ptr(mult), _ptr(rows) if want_rows else None, C.byref(bad))
        if log_capacity is None:
            rc = self._lib.kzg_lookup_multiplicities(*args)
        else:
            rc = self._lib.kzg_lookup_multiplicities_cap(*args, log_capacity)
        self._gp_status(rc, bad)
        return mult, rows

    def lookup_multiplicities_device(self, d_table, n_table, d_lookups, n, k, d_out_mult, d_out_rows=None, stride=None):
        bad = C.c_size_t(0)
        self._gp_status(self._lib.kzg_lookup_multiplicities_device(self._h, C.c_void_p(d_table), n_table, C.c_void_p(d_lookups), n, k,
                                                                   n if stride is None else stride, C.c_void_p(d_out_mult),
                                                                   None if d_out_rows is None else C.c_void_p(d_out_rows),
                                                                   C.byref(bad)), bad)

    # -- the quotient of a permutation argument on the coset 7 H_N --
    def _pq_check(self, rc):
        if rc != KZG_OK:
            raise self._error(rc)  # with kzg_last_error: it says which constraint or argument the status is about

    def coset_extend_limbs(self, cols, log_out, form=KZG_EXTEND_VALUES, n=None):
        """kzg_coset_extend: cols a (batch, stride, 4) array whose first n rows per column count (n=None: all) -> (batch, N, 4)"""
        a, batch, stride, n = self._columns(cols, n)
        out = np.zeros((batch, 1 << log_out, 4), dtype=np.uint64)
        self._pq_check(self._lib.kzg_coset_extend(self._h, _ptr(a), n, batch, stride, form, log_out, _ptr(out)))
        return out

    def coset_extend_device(self, d_in, n, batch, log_out, d_out, form=KZG_EXTEND_VALUES, stride=None):
        self._pq_check(self._lib.kzg_coset_extend_device(self._h, C.c_void_p(d_in), n, batch, n if stride is None else stride, form, log_out,
                                                 C.c_void_p(d_out)))

    def _pq_scalars(self, shifts, alpha, beta, gamma, t):
        sh, bl, gl = self._perm_scalars(shifts, beta, gamma, t)
        return sh, alpha.limbs(), bl, gl

    def permutation_constraints_coset_limbs(self, wires_ext, sigmas_ext, z_ext, n, shifts, alpha, beta, gamma, gate=None, N=None):
        """kzg_permutation_constraints_coset: wires_ext, sigmas_ext (t, stride, 4) arrays of values on the coset, z_ext (N, 4)
        -> Num / Z_H on the coset, an (N, 4) array"""
        z = np.ascontiguousarray(z_ext, dtype=np.uint64).reshape(-1, 4)
        a, t, stride, N = self._columns(wires_ext, z.shape[0] if N is None else N)
        b = np.ascontiguousarray(sigmas_ext, dtype=np.uint64).reshape(t, stride, 4)
        g = None if gate is None else np.ascontiguousarray(gate, dtype=np.uint64).reshape(N, 4)
        sh, al, bl, gl = self._pq_scalars(shifts, alpha, beta, gamma, t)
        out = np.zeros((N, 4), dtype=np.uint64)
        self._pq_check(self._lib.kzg_permutation_constraints_coset(self._h, _ptr(a), _ptr(b), _ptr(z), n, N // n, t, stride, _ptr(sh), _ptr(al),
                                                           _ptr(bl), _ptr(gl), None if g is None else _ptr(g), _ptr(out)))
        return out

    def permutation_constraints_coset_device(self, d_wires, d_sigmas, d_z, n, rot, t, shifts, alpha, beta, gamma, d_out, d_gate=None,
                                             stride=None):
        sh, al, bl, gl = self._pq_scalars(shifts, alpha, beta, gamma, t)
        self._pq_check(self._lib.kzg_permutation_constraints_coset_device(
            self._h, C.c_void_p(d_wires), C.c_void_p(d_sigmas), C.c_void_p(d_z), n, rot, t, n * rot if stride is None else stride,
            _ptr(sh), _ptr(al), _ptr(bl), _ptr(gl), C.c_void_p(d_gate), C.c_void_p(d_out)))

    def vanishing_quotient_limbs(self, num_coset, n, already_divided=False):
        """kzg_vanishing_quotient: N values of Num on the coset -> the (N - n, 4) coefficients of Num / (X^n - 1)"""
        a = np.ascontiguousarray(num_coset, dtype=np.uint64).reshape(-1, 4)
        N = a.shape[0]
        out = np.zeros((max(N - n, 0), 4), dtype=np.uint64)
        self._pq_check(self._lib.kzg_vanishing_quotient(self._h, _ptr(a), N, n, 1 if already_divided else 0, _ptr(out)))
        return out

    def vanishing_quotient_device(self, d_num, N, n, d_out, already_divided=False):
        self._pq_check(self._lib.kzg_vanishing_quotient_device(self._h, C.c_void_p(d_num), N, n, 1 if already_divided else 0,
                                                       C.c_void_p(d_out)))

    def permutation_quotient(self, wires, sigmas, z, shifts, alpha, beta, gamma, log_ext, gate=None, n=None, want_coeffs=True,
                             want_commitments=True):
        """kzg_permutation_quotient: wires, sigmas (t, stride, 4) arrays, z (n, 4) -> (T's coefficients (N - n, 4) or None, the list
        of its chunks' commitments or None)"""
        a, t, stride, n = self._columns(wires, n)
        b = np.ascontiguousarray(sigmas, dtype=np.uint64).reshape(t, stride, 4)
        zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 4)
        assert zz.shape[0] >= n
        N = n << log_ext
        g = None if gate is None else np.ascontiguousarray(gate, dtype=np.uint64).reshape(N, 4)
        sh, al, bl, gl = self._pq_scalars(shifts, alpha, beta, gamma, t)
        coeffs = np.zeros((N - n, 4), dtype=np.uint64) if want_coeffs else None
        p1s = np.zeros(((1 << log_ext) - 1, 18), dtype=np.uint64) if want_commitments else None
        self._pq_check(self._lib.kzg_permutation_quotient(self._h, _ptr(a), _ptr(b), _ptr(zz), n, t, stride, _ptr(sh), _ptr(al), _ptr(bl),
                                                  _ptr(gl), None if g is None else _ptr(g), log_ext,
                                                  None if coeffs is None else _ptr(coeffs), None if p1s is None else _ptr(p1s)))
        return coeffs, None if p1s is None else [G1Point(p) for p in p1s]

    # -- a circuit's key resident on the device: the quotient with the arithmetic gate built in --
    def circuit_create(self, q_lin, q_mul, q_const, sigmas, shifts, log_ext, n=None, want_key=True):
        """kzg_circuit_create: q_lin, sigmas (t, stride, 4) arrays whose first n rows per column count (n=None: all), q_mul and
        q_const (n, 4) arrays, shifts t Scalars -> a Circuit.  want_key: commit the 2 t + 2 columns (needs the SRS); they are
        Circuit.key in the order q_lin[0..t), q_mul, q_const, sigma[0..t)"""
        a, t, stride, n = self._columns(q_lin, n)
        b = np.ascontiguousarray(sigmas, dtype=np.uint64).reshape(t, stride, 4)
        qm = np.ascontiguousarray(q_mul, dtype=np.uint64).reshape(-1, 4)
        qc = np.ascontiguousarray(q_const, dtype=np.uint64).reshape(-1, 4)
        assert qm.shape[0] >= n and qc.shape[0] >= n
        sh = np.ascontiguousarray([k.limbs() for k in shifts], dtype=np.uint64).reshape(-1, 4)
        assert sh.shape[0] == t, "one coset shift per column"
        p1s = np.zeros((2 * t + 2, 18), dtype=np.uint64) if want_key else None
        h = C.c_void_p()
        self._pq_check(self._lib.kzg_circuit_create(self._h, _ptr(a), _ptr(qm), _ptr(qc), _ptr(b), n, t, stride, _ptr(sh), log_ext,
                                                    None if p1s is None else _ptr(p1s), C.byref(h)))
        return Circuit(self, h, n, t, log_ext, None if p1s is None else [G1Point(p) for p in p1s])

    def circuit_create_lookup(self, q_lin, q_mul, q_const, sigmas, shifts, log_ext, table, q_lookup, n=None, want_key=True):
        """kzg_circuit_create_lookup: circuit_create's arguments, table a (c, table_stride, 4) array whose first n rows per column
        count and q_lookup an (n, 4) array -> a Circuit with c table columns; its key has 2 t + c + 3 commitments, circuit_create's
        and then tab[0..c), q_K"""
        a, t, stride, n = self._columns(q_lin, n)
        b = np.ascontiguousarray(sigmas, dtype=np.uint64).reshape(t, stride, 4)
        qm = np.ascontiguousarray(q_mul, dtype=np.uint64).reshape(-1, 4)
        qc = np.ascontiguousarray(q_const, dtype=np.uint64).reshape(-1, 4)
        tb = np.ascontiguousarray(table, dtype=np.uint64)
        assert tb.ndim == 3 and tb.shape[2] == 4 and tb.shape[1] >= n
        qk = np.ascontiguousarray(q_lookup, dtype=np.uint64).reshape(-1, 4)
        assert qm.shape[0] >= n and qc.shape[0] >= n and qk.shape[0] >= n
        sh = np.ascontiguousarray([k.limbs() for k in shifts], dtype=np.uint64).reshape(-1, 4)
        assert sh.shape[0] == t, "one coset shift per column"
        c = tb.shape[0]
        p1s = np.zeros((2 * t + c + 3, 18), dtype=np.uint64) if want_key else None
        h = C.c_void_p()
        self._pq_check(self._lib.kzg_circuit_create_lookup(self._h, _ptr(a), _ptr(qm), _ptr(qc), _ptr(b), n, t, stride, _ptr(sh), log_ext,
                                                           _ptr(tb), c, tb.shape[1], _ptr(qk), None if p1s is None else _ptr(p1s),
                                                           C.byref(h)))
        circ = Circuit(self, h, n, t, log_ext, None if p1s is None else [G1Point(p) for p in p1s])
        circ.c = c
        return circ

    def circuit_create_custom(self, q_lin, q_mul, q_const, sigmas, shifts, log_ext, q_custom, exponents, n=None, want_key=True,
                              exponents_next=None):
        """kzg_circuit_create_custom: circuit_create's arguments, q_custom a (g, custom_stride, 4) array whose first n rows per
        column count and exponents a (g, t) array of bytes in 0..7 -> a Circuit with g custom terms; its key has 2 t + 2 + g
        commitments, circuit_create's and then qx[0..g).  With exponents_next, a second (g, t) array:
        kzg_circuit_create_custom_next, a next-row circuit (Circuit.rho wires are read at the row after too)"""
        a, t, stride, n = self._columns(q_lin, n)
        b = np.ascontiguousarray(sigmas, dtype=np.uint64).reshape(t, stride, 4)
        qm = np.ascontiguousarray(q_mul, dtype=np.uint64).reshape(-1, 4)
        qc = np.ascontiguousarray(q_const, dtype=np.uint64).reshape(-1, 4)
        qx = np.ascontiguousarray(q_custom, dtype=np.uint64)
        assert qx.ndim == 3 and qx.shape[2] == 4 and qx.shape[1] >= n
        assert qm.shape[0] >= n and qc.shape[0] >= n
        g = qx.shape[0]
        ex = np.ascontiguousarray(exponents, dtype=np.uint8).reshape(g, t)
        sh = np.ascontiguousarray([k.limbs() for k in shifts], dtype=np.uint64).reshape(-1, 4)
        assert sh.shape[0] == t, "one coset shift per column"
        p1s = np.zeros((2 * t + 2 + g, 18), dtype=np.uint64) if want_key else None
        h = C.c_void_p()
        if exponents_next is None:
            self._pq_check(self._lib.kzg_circuit_create_custom(self._h, _ptr(a), _ptr(qm), _ptr(qc), _ptr(b), n, t, stride, _ptr(sh),
                                                               log_ext, _ptr(qx), g, qx.shape[1], _ptr(ex),
                                                               None if p1s is None else _ptr(p1s), C.byref(h)))
        else:
            exn = np.ascontiguousarray(exponents_next, dtype=np.uint8).reshape(g, t)
            self._pq_check(self._lib.kzg_circuit_create_custom_next(self._h, _ptr(a), _ptr(qm), _ptr(qc), _ptr(b), n, t, stride, _ptr(sh),
                                                                    log_ext, _ptr(qx), g, qx.shape[1], _ptr(ex), _ptr(exn),
                                                                    None if p1s is None else _ptr(p1s), C.byref(h)))
        circ = Circuit(self, h, n, t, log_ext, None if p1s is None else [G1Point(p) for p in p1s])
        circ.g, circ.exponents = g, ex
        if exponents_next is not None:
            circ.exponents_next, circ.rho = exn, int(np.count_nonzero(exn.any(axis=0)))
        return circ

    def circuit_create_custom_next(self, q_lin, q_mul, q_const, sigmas, shifts, log_ext, q_custom, exponents, exponents_next, n=None,
                                   want_key=True):
        """kzg_circuit_create_custom_next: circuit_create_custom with the (g, t) next-row exponents p'"""
        return self.circuit_create_custom(q_lin, q_mul, q_const, sigmas, shifts, log_ext, q_custom, exponents, n=n, want_key=want_key,
                                          exponents_next=exponents_next)

    # -- zero-knowledge blinding --
    def blind_evaluations_limbs(self, evals, blinders, n=None):
        """kzg_blind_evaluations: evals a (k, stride, 4) array of values over H whose first n rows per column count, blinders a
        (k, nb, 4) array (nb <= 3) -> the (k, n + nb, 4) coefficients of f + b (X^n - 1)"""
        a, k, stride, n = self._columns(evals, n)
        b = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(k, -1, 4)
        nb = b.shape[1]
        out = np.zeros((k, n + nb, 4), dtype=np.uint64)
        self._pq_check(self._lib.kzg_blind_evaluations(self._h, _ptr(a), n, k, stride, _ptr(b), nb, _ptr(out), n + nb))
        return out

    def commit_evaluations_blinded(self, evals, blinders, n=None):
        """kzg_commit_evaluations_blinded: as blind_evaluations_limbs -> the k commitments of the blinded columns"""
        a, k, stride, n = self._columns(evals, n)
        b = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(k, -1, 4)
        p1s = np.zeros((k, 18), dtype=np.uint64)
        self._pq_check(self._lib.kzg_commit_evaluations_blinded(self._h, _ptr(a), n, k, stride, _ptr(b), b.shape[1], _ptr(p1s)))
        return [G1Point(p) for p in p1s]

    # -- multilinear openings (Gemini / HyperKZG): 2^ell values on the hypercube, u a list of ell Scalars -------------------
    # values: (n, 4) uint64 blst_fr images; the pyramid: f_1 .. f_ell packed, level i at offset n - (n >> (i - 1))
    @staticmethod
    def _ml_values(evals):
        a = np.ascontiguousarray(evals, dtype=np.uint64).reshape(-1, 4)
        ell = max(a.shape[0].bit_length() - 1, 0)
        assert a.shape[0] == 1 << ell
        return a, ell

    def ml_fold(self, evals, us):
        """kzg_ml_fold: the pyramid as an (n - 1, 4) array"""
        a, ell = self._ml_values(evals)
        assert len(us) == ell
        out = np.zeros((max(a.shape[0] - 1, 1), 4), dtype=np.uint64)
        _check(self._lib.kzg_ml_fold(self._h, _ptr(a), ell, _ptr(_scalar_rows(us)), _ptr(out)), self._h)
        return out[:a.shape[0] - 1].copy()

    def ml_evaluate(self, evals, us):
        """kzg_ml_evaluate: f~(u)"""
        a, ell = self._ml_values(evals)
        assert len(us) == ell
        v = np.zeros(4, dtype=np.uint64)
        _check(self._lib.kzg_ml_evaluate(self._h, _ptr(a), ell, _ptr(_scalar_rows(us)), _ptr(v)), self._h)
        return Scalar.from_limbs(v)

    def ml_fold_device(self, d_evals, ell, us, d_pyramid):
        """kzg_ml_fold_device: fills the n - 1 values at d_pyramid, returns v = f~(u)"""
        v = np.zeros(4, dtype=np.uint64)
        _check(self._lib.kzg_ml_fold_device(self._h, C.c_void_p(d_evals), ell, _ptr(_scalar_rows(us)), C.c_void_p(d_pyramid),
                                            _ptr(v)), self._h)
        return Scalar.from_limbs(v)

    def ml_commit_folds_device(self, d_pyramid, ell):
        """kzg_ml_commit_folds_device: [C_1 .. C_(ell-1)]"""
        out = np.zeros((max(ell - 1, 1), 18), dtype=np.uint64)
        _check(self._lib.kzg_ml_commit_folds_device(self._h, C.c_void_p(d_pyramid), ell, _ptr(out)), self._h)
        return [G1Point(out[i].copy()) for i in range(max(ell - 1, 0))]

    def ml_evaluations_device(self, d_evals, d_pyramid, ell, r):
        """kzg_ml_evaluations_device: ys[i] = [f_i(r), f_i(-r), f_i(r^2)], i < ell"""
        ys = np.zeros((3 * max(ell, 1), 4), dtype=np.uint64)
        _check(self._lib.kzg_ml_evaluations_device(self._h, C.c_void_p(d_evals), C.c_void_p(d_pyramid), ell, _ptr(r.limbs()),
                                                   _ptr(ys)), self._h)
        return [[Scalar.from_limbs(ys[3 * i + p]) for p in range(3)] for i in range(ell)]

    def ml_open_device(self, d_evals, d_pyramid, ell, r, gamma):
        """kzg_ml_open_device: W"""
        out = np.zeros(18, dtype=np.uint64)
        _check(self._lib.kzg_ml_open_device(self._h, C.c_void_p(d_evals), C.c_void_p(d_pyramid), ell, _ptr(r.limbs()),
                                            _ptr(gamma.limbs()), _ptr(out)), self._h)
        return G1Point(out)

    def ml_open(self, evals, us, r, gamma):
        """kzg_ml_open: (v, [C_1 .. C_(ell-1)], ys, W) with ys[i] = [f_i(r), f_i(-r), f_i(r^2)]"""
        a, ell = self._ml_values(evals)
        assert len(us) == ell
        v = np.zeros(4, dtype=np.uint64)
        folds = np.zeros((max(ell - 1, 1), 18), dtype=np.uint64)
        ys = np.zeros((3 * max(ell, 1), 4), dtype=np.uint64)
        out = np.zeros(18, dtype=np.uint64)
        _check(self._lib.kzg_ml_open(self._h, _ptr(a), ell, _ptr(_scalar_rows(us)), _ptr(r.limbs()), _ptr(gamma.limbs()), _ptr(v),
                                     _ptr(folds), _ptr(ys), _ptr(out)), self._h)
        return (Scalar.from_limbs(v), [G1Point(folds[i].copy()) for i in range(max(ell - 1, 0))],
                [[Scalar.from_limbs(ys[3 * i + p]) for p in range(3)] for i in range(ell)], G1Point(out))

    # -- device-resident, pipelined --
    def num_slots(self):
        return int(self._lib.kzg_num_slots(self._h))

    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        _check(self._lib.kzg_dev_alloc(self._h, nbytes, C.byref(p)), self._h)
        return p.value

    def dev_free(self, dptr):
        _check(self._lib.kzg_dev_free(self._h, C.c_void_p(dptr)), self._h)

    def dev_upload(self, dptr, array):
        a = np.ascontiguousarray(array)
        _check(self._lib.kzg_dev_upload(self._h, C.c_void_p(dptr), _ptr(a), a.nbytes), self._h)

    def commit_submit(self, slot, dptr, n):
        _check(self._lib.kzg_commit_submit(self._h, slot, C.c_void_p(dptr), n), self._h)

    def open_submit(self, slot, dptr, n, z, y):
        zl, yl = z.limbs(), y.limbs()
        _check(self._lib.kzg_open_submit(self._h, slot, C.c_void_p(dptr), n, _ptr(zl), _ptr(yl)), self._h)

    def wait(self, slot):
        out = np.zeros(18, dtype=np.uint64)
        _check(self._lib.kzg_wait(self._h, slot, _ptr(out)), self._h)
        return G1Point(out)

    def set_max_batch(self, b):
        _check(self._lib.kzg_set_max_batch(self._h, b), self._h)
        return int(self._lib.kzg_max_batch(self._h))

    def max_batch(self):
        return int(self._lib.kzg_max_batch(self._h))

    def commit_batch_submit(self, slot, dptr, n, batch, stride=None):
        _check(self._lib.kzg_commit_batch_submit(self._h, slot, C.c_void_p(dptr), n, batch, n if stride is None else stride),
               self._h)

    def wait_batch(self, slot, batch):
        out = np.zeros((batch, 18), dtype=np.uint64)
        _check(self._lib.kzg_wait_batch(self._h, slot, _ptr(out), batch), self._h)
        return [G1Point(out[i]) for i in range(batch)]

    def open_batch_limbs(self, polys, zs, ys):
        """Batched generate_proof: returns a list of G1Point or KzgError per polynomial."""
        polys = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in polys]
        n, b = polys[0].shape[0], len(polys)
        assert all(p.shape[0] == n for p in polys) and len(zs) == b and len(ys) == b
        flat = np.concatenate(polys)
        zl = np.ascontiguousarray(np.stack([z.limbs() for z in zs]))
        yl = np.ascontiguousarray(np.stack([y.limbs() for y in ys]))
        dptr = self.dev_alloc(flat.nbytes)
        try:
            self.dev_upload(dptr, flat)
            _check(self._lib.kzg_open_batch_submit(self._h, 0, C.c_void_p(dptr), n, b, n, _ptr(zl), _ptr(yl)), self._h)
            out = np.zeros((b, 18), dtype=np.uint64)
            st = np.zeros(b, dtype=np.int32)
            _check(self._lib.kzg_wait_open_batch(self._h, 0, _ptr(out), _ptr(st), b), self._h)
        finally:
            self.dev_free(dptr)
        res = []
        for i in range(b):
            if st[i] == KZG_OK:
                res.append(G1Point(out[i]))
            else:
                res.append(KzgError(int(st[i]), self._lib.kzg_strerror(int(st[i])).decode()))
        return res

    # -- host-pointer batches (every kind of context) --
    @staticmethod
    def _stack(polys):
        """list of (n, 4) arrays, or one (batch, n, 4) array -> contiguous (batch, n, 4) uint64"""
        a = np.asarray(polys, dtype=np.uint64) if not isinstance(polys, np.ndarray) else polys
        if a.ndim != 3:
            a = np.stack([np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in polys])
        return np.ascontiguousarray(a, dtype=np.uint64)

    def commit_batch_host(self, polys):
        """kzg_commit_batch: one call for a list of equally long polynomials in host memory."""
        flat = self._stack(polys)
        b, n = flat.shape[0], flat.shape[1]
        out = np.zeros((b, 18), dtype=np.uint64)
        _check(self._lib.kzg_commit_batch(self._h, _ptr(flat), n, b, n, _ptr(out)), self._h)
        return [G1Point(out[i]) for i in range(b)]

    def open_batch_host(self, polys, zs, ys):
        """kzg_open_batch: returns a list of G1Point or KzgError per polynomial."""
        flat = self._stack(polys)
        b, n = flat.shape[0], flat.shape[1]
        assert len(zs) == b and len(ys) == b
        zl = np.ascontiguousarray(np.stack([z.limbs() for z in zs]))
        yl = np.ascontiguousarray(np.stack([y.limbs() for y in ys]))
        out = np.zeros((b, 18), dtype=np.uint64)
        st = np.zeros(b, dtype=np.int32)
        _check(self._lib.kzg_open_batch(self._h, _ptr(flat), n, b, n, _ptr(zl), _ptr(yl), _ptr(out), _ptr(st)), self._h)
        return [G1Point(out[i]) if st[i] == KZG_OK else KzgError(int(st[i]), self._lib.kzg_strerror(int(st[i])).decode())
                for i in range(b)]

    def commit_batch_limbs(self, polys):
        """Commits several coefficient arrays (each (n, 4) uint64, same n) in one batched pass."""
        polys = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in polys]
        n = polys[0].shape[0]
        assert all(p.shape[0] == n for p in polys)
        flat = np.concatenate(polys)
        dptr = self.dev_alloc(flat.nbytes)
        try:
            self.dev_upload(dptr, flat)
            self.commit_batch_submit(0, dptr, n, len(polys))
            return self.wait_batch(0, len(polys))
        finally:
            self.dev_free(dptr)

    # -- measurement --
    def set_timing(self, enabled):
        _check(self._lib.kzg_set_timing(self._h, 1 if enabled else 0))

    def times(self, slot):
        t = KernelTimes()
        _check(self._lib.kzg_get_times(self._h, slot, C.byref(t)))
        return {n: getattr(t, n) for n, _ in KernelTimes._fields_}


# ---------------------------------------------------------------------------------------------
# SetupArtifactsGenerator: reference src/trusted_setup.rs:9-29 / 37-78.  `take(n)` materialises the
# first n artifacts -- on the device, G1 side -- and returns the engine that now holds them; the
# reference's `Vec<SetupArtifact>` argument of commit / generate_proof becomes that engine.
# ---------------------------------------------------------------------------------------------
class Circuit:
    """A circuit's key resident on the device (kzg_circuit_create).  key: the commitments of its 2 t + 2 columns, or None.  The
    handle lives until close() or until its Engine is closed, whichever comes first."""

    def __init__(self, engine, handle, n, t, log_ext, key):
        self._eng, self._c = engine, handle
        self.n, self.t, self.log_ext, self.key = n, t, log_ext, key
        self.c = 0  # table columns (circuit_create_lookup)
        self.g, self.exponents = 0, None  # custom terms and their (g, t) exponents (circuit_create_custom)
        self.rho, self.exponents_next = 0, None  # wires read at the next row and p' (circuit_create_custom_next)

    def close(self):
        if getattr(self, "_c", None) and getattr(self._eng, "_h", None):
            self._eng._pq_check(self._eng._lib.kzg_circuit_destroy(self._eng._h, self._c))
        self._c = None

    def quotient(self, wires, z, alpha, beta, gamma, public_inputs=None, gate=None, n=None, want_coeffs=True, want_commitments=True,
                 engine=None):
        """kzg_circuit_quotient: wires a (t, stride, 4) array, z (n, 4), public_inputs None or (n, 4), gate None or the (N, 4)
        values of the caller's own term on the coset -> (T's coefficients (N - n, 4) or None, the list of its chunks' commitments
        or None).  engine: the context the call is made on (the circuit's own unless given)"""
        e = self._eng if engine is None else engine
        a, t, stride, n = e._columns(wires, self.n if n is None else n)
        assert t == self.t and n == self.n
        zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 4)
        assert zz.shape[0] >= n
        N = n << self.log_ext
        pi = None if public_inputs is None else np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1, 4)
        assert pi is None or pi.shape[0] >= n
        g = None if gate is None else np.ascontiguousarray(gate, dtype=np.uint64).reshape(N, 4)
        al, bl, gl = alpha.limbs(), beta.limbs(), gamma.limbs()
        coeffs = np.zeros((N - n, 4), dtype=np.uint64) if want_coeffs else None
        p1s = np.zeros(((1 << self.log_ext) - 1, 18), dtype=np.uint64) if want_commitments else None
        e._pq_check(e._lib.kzg_circuit_quotient(e._h, self._c, _ptr(a), stride, _ptr(zz), None if pi is None else _ptr(pi), _ptr(al),
                                                _ptr(bl), _ptr(gl), None if g is None else _ptr(g),
                                                None if coeffs is None else _ptr(coeffs), None if p1s is None else _ptr(p1s)))
        return coeffs, None if p1s is None else [G1Point(p) for p in p1s]

    def quotient_device(self, d_wires, d_z, alpha, beta, gamma, d_out_coeffs, d_public_inputs=None, d_gate=None, stride=None):
        """kzg_circuit_quotient_device on kzg_dev_alloc buffers: T's N - n coefficients land in d_out_coeffs"""
        e = self._eng
        al, bl, gl = alpha.limbs(), beta.limbs(), gamma.limbs()
        e._pq_check(e._lib.kzg_circuit_quotient_device(e._h, self._c, C.c_void_p(d_wires), self.n if stride is None else stride,
                                                       C.c_void_p(d_z), C.c_void_p(d_public_inputs), _ptr(al), _ptr(bl), _ptr(gl),
                                                       C.c_void_p(d_gate), C.c_void_p(d_out_coeffs)))

    # -- the last round: linearise, open once --
    def _open_inputs(self, e, wires, z, public_inputs, t_coeffs, n):
        a, t, stride, n = e._columns(wires, self.n if n is None else n)
        assert t == self.t and n == self.n
        zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 4)
        pi = None if public_inputs is None else np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1, 4)
        tc = np.ascontiguousarray(t_coeffs, dtype=np.uint64).reshape(-1, 4)
        assert zz.shape[0] >= n and (pi is None or pi.shape[0] >= n) and tc.shape[0] >= (n << self.log_ext) - n
        return a, stride, zz, pi, tc

    def _split_evals(self, ev):
        t = self.t
        sc = [Scalar.from_limbs(row) for row in ev]
        return sc[:t], sc[t:2 * t - 1], sc[2 * t - 1]

    def open(self, wires, z, t_coeffs, alpha, beta, gamma, zeta, v, public_inputs=None, n=None, engine=None):
        """kzg_circuit_open: wires, z, public_inputs as quotient() takes them, t_coeffs the (N - n, 4) coefficients it returned ->
        ((the t values f_j(zeta), the t - 1 values sigma_j(zeta), z(zeta w)), the proof).  The challenges are taken as given:
        zeta is fixed after T's commitments and v after the values; nothing is hashed here."""
        e = self._eng if engine is None else engine
        a, stride, zz, pi, tc = self._open_inputs(e, wires, z, public_inputs, t_coeffs, n)
        ch = [x.limbs() for x in (alpha, beta, gamma, zeta, v)]
        ev, p1 = np.zeros((2 * self.t, 4), dtype=np.uint64), np.zeros(18, dtype=np.uint64)
        e._pq_check(e._lib.kzg_circuit_open(e._h, self._c, _ptr(a), stride, _ptr(zz), None if pi is None else _ptr(pi), _ptr(tc),
                                            _ptr(ch[0]), _ptr(ch[1]), _ptr(ch[2]), _ptr(ch[3]), _ptr(ch[4]), _ptr(ev), _ptr(p1)))
        return self._split_evals(ev), G1Point(p1)

    def open_device(self, d_wires, d_z, d_t_coeffs, alpha, beta, gamma, zeta, v, d_public_inputs=None, stride=None):
        """kzg_circuit_open_device on kzg_dev_alloc buffers (d_t_coeffs: what quotient_device wrote) -> as open()"""
        e = self._eng
        ch = [x.limbs() for x in (alpha, beta, gamma, zeta, v)]
        ev, p1 = np.zeros((2 * self.t, 4), dtype=np.uint64), np.zeros(18, dtype=np.uint64)
        e._pq_check(e._lib.kzg_circuit_open_device(e._h, self._c, C.c_void_p(d_wires), self.n if stride is None else stride,
                                                   C.c_void_p(d_z), C.c_void_p(d_public_inputs), C.c_void_p(d_t_coeffs), _ptr(ch[0]),
                                                   _ptr(ch[1]), _ptr(ch[2]), _ptr(ch[3]), _ptr(ch[4]), _ptr(ev), _ptr(p1)))
        return self._split_evals(ev), G1Point(p1)

    def linearise(self, wires, z, t_coeffs, alpha, beta, gamma, zeta, public_inputs=None, n=None, engine=None):
        """kzg_circuit_linearise (test hook, no SRS) -> (the evaluations as open() returns them, r's (n, 4) coefficients)"""
        e = self._eng if engine is None else engine
        a, stride, zz, pi, tc = self._open_inputs(e, wires, z, public_inputs, t_coeffs, n)
        ch = [x.limbs() for x in (alpha, beta, gamma, zeta)]
        ev, r = np.zeros((2 * self.t, 4), dtype=np.uint64), np.zeros((self.n, 4), dtype=np.uint64)
        e._pq_check(e._lib.kzg_circuit_linearise(e._h, self._c, _ptr(a), stride, _ptr(zz), None if pi is None else _ptr(pi), _ptr(tc),
                                                 _ptr(ch[0]), _ptr(ch[1]), _ptr(ch[2]), _ptr(ch[3]), _ptr(ev), _ptr(r)))
        return self._split_evals(ev), r

    # -- the blinded rounds --
    def _prove(self, fn, e, wires_arg, stride, public_inputs, blinders, size=None):
        assert self.key is not None, "prove: the circuit was created without its key commitments"
        rows = np.ascontiguousarray(np.stack([c.p1 for c in self.key]), dtype=np.uint64)
        pub = None
        if public_inputs is not None and len(public_inputs):
            pub = np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1, 4)
        bl = None if blinders is None else np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1, 4)
        assert bl is None or bl.shape[0] == 2 * self.t + 3 + (1 << self.log_ext) - 2
        out = np.zeros(circuit_proof_size(self.t, self.log_ext) if size is None else size, dtype=np.uint8)
        e._pq_check(fn(e._h, self._c, _ptr(rows), wires_arg, stride, _ptr(pub) if pub is not None else None,
                       0 if pub is None else pub.shape[0], _ptr(bl) if bl is not None else None, _ptr(out)))
        return out.tobytes()

    def prove(self, wires, public_inputs=None, blinders=None, n=None, engine=None):
        """kzg_circuit_prove: wires a (t, stride, 4) array, public_inputs None or the (n_public, 4) values of rows
        0 .. n_public - 1, blinders None (a plain proof: NOT zero-knowledge) or the array of blinders() -> the proof bytes
        (circuit_proof_size of them), every challenge derived from the transcript inside the call"""
        e = self._eng if engine is None else engine
        a, t, stride, n = e._columns(wires, self.n if n is None else n)
        assert t == self.t and n == self.n
        return self._prove(e._lib.kzg_circuit_prove, e, _ptr(a), stride, public_inputs, blinders)

    def prove_device(self, d_wires, public_inputs=None, blinders=None, stride=None):
        """kzg_circuit_prove_device: the wires in a device buffer of the circuit's (single-device) context"""
        e = self._eng
        return self._prove(e._lib.kzg_circuit_prove_device, e, C.c_void_p(d_wires), self.n if stride is None else stride,
                           public_inputs, blinders)

    def blinders(self):
        """kzg_circuit_blinders: a fresh (2 t + 3 + e - 2, 4) blinder array from the OS CSPRNG"""
        return circuit_blinders(self.t, self.log_ext)

    def blinded_sizes(self):
        """kzg_circuit_blinded_sizes -> (blinders in the array, L_T = coefficients of the blinded quotient)"""
        return circuit_blinded_sizes(self.n, self.t, self.log_ext)

    def quotient_blinded(self, wires, z, alpha, beta, gamma, blinders, public_inputs=None, n=None, want_coeffs=True,
                         want_commitments=True, engine=None):
        """kzg_circuit_quotient_blinded: as quotient() without a gate, blinders the array of blinders() -> (T~'s (L_T, 4)
        coefficients or None, the commitments of its e - 1 blinded chunks or None)"""
        e = self._eng if engine is None else engine
        a, t, stride, n = e._columns(wires, self.n if n is None else n)
        assert t == self.t and n == self.n
        zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 4)
        pi = None if public_inputs is None else np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1, 4)
        assert zz.shape[0] >= n and (pi is None or pi.shape[0] >= n)
        b = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1, 4)
        ext = 1 << self.log_ext
        assert b.shape[0] == 2 * t + 3 + ext - 2
        al, bl, gl = alpha.limbs(), beta.limbs(), gamma.limbs()
        coeffs = np.zeros(((ext - 1) * n + t + 3, 4), dtype=np.uint64) if want_coeffs else None
        p1s = np.zeros((ext - 1, 18), dtype=np.uint64) if want_commitments else None
        e._pq_check(e._lib.kzg_circuit_quotient_blinded(e._h, self._c, _ptr(a), stride, _ptr(zz), None if pi is None else _ptr(pi),
                                                        _ptr(al), _ptr(bl), _ptr(gl), _ptr(b),
                                                        None if coeffs is None else _ptr(coeffs), None if p1s is None else _ptr(p1s)))
        return coeffs, None if p1s is None else [G1Point(p) for p in p1s]

    def quotient_blinded_device(self, d_wires, d_z, alpha, beta, gamma, blinders, d_out_coeffs, d_public_inputs=None, stride=None,
                                want_commitments=True):
        """kzg_circuit_quotient_blinded_device on kzg_dev_alloc buffers: T~'s L_T coefficients land in d_out_coeffs -> the
        commitments of its blinded chunks or None"""
        e = self._eng
        b = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1, 4)
        assert b.shape[0] == 2 * self.t + 3 + (1 << self.log_ext) - 2
        al, bl, gl = alpha.limbs(), beta.limbs(), gamma.limbs()
        p1s = np.zeros(((1 << self.log_ext) - 1, 18), dtype=np.uint64) if want_commitments else None
        e._pq_check(e._lib.kzg_circuit_quotient_blinded_device(e._h, self._c, C.c_void_p(d_wires), self.n if stride is None else stride,
                                                               C.c_void_p(d_z), C.c_void_p(d_public_inputs), _ptr(al), _ptr(bl),
                                                               _ptr(gl), _ptr(b), C.c_void_p(d_out_coeffs),
                                                               None if p1s is None else _ptr(p1s)))
        return None if p1s is None else [G1Point(p) for p in p1s]

    def open_blinded(self, wires, z, t_coeffs, alpha, beta, gamma, zeta, v, blinders, public_inputs=None, n=None, engine=None):
        """kzg_circuit_open_blinded: as open(), t_coeffs the (L_T, 4) coefficients of quotient_blinded() and blinders the same
        array -> ((the t values f~_j(zeta), the t - 1 values sigma_j(zeta), z~(zeta w)), the proof)"""
        e = self._eng if engine is None else engine
        a, t, stride, n = e._columns(wires, self.n if n is None else n)
        assert t == self.t and n == self.n
        zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 4)
        pi = None if public_inputs is None else np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1, 4)
        tc = np.ascontiguousarray(t_coeffs, dtype=np.uint64).reshape(-1, 4)
        b = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1, 4)
        ext = 1 << self.log_ext
        assert zz.shape[0] >= n and (pi is None or pi.shape[0] >= n) and tc.shape[0] >= (ext - 1) * n + t + 3
        assert b.shape[0] == 2 * t + 3 + ext - 2
        ch = [x.limbs() for x in (alpha, beta, gamma, zeta, v)]
        ev, p1 = np.zeros((2 * self.t, 4), dtype=np.uint64), np.zeros(18, dtype=np.uint64)
        e._pq_check(e._lib.kzg_circuit_open_blinded(e._h, self._c, _ptr(a), stride, _ptr(zz), None if pi is None else _ptr(pi),
                                                    _ptr(tc), _ptr(ch[0]), _ptr(ch[1]), _ptr(ch[2]), _ptr(ch[3]), _ptr(ch[4]), _ptr(b),
                                                    _ptr(ev), _ptr(p1)))
        return self._split_evals(ev), G1Point(p1)

    def open_blinded_device(self, d_wires, d_z, d_t_coeffs, alpha, beta, gamma, zeta, v, blinders, d_public_inputs=None, stride=None):
        """kzg_circuit_open_blinded_device on kzg_dev_alloc buffers (d_t_coeffs: what quotient_blinded_device wrote) -> as
        open_blinded()"""
        e = self._eng
        b = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1, 4)
        assert b.shape[0] == 2 * self.t + 3 + (1 << self.log_ext) - 2
        ch = [x.limbs() for x in (alpha, beta, gamma, zeta, v)]
        ev, p1 = np.zeros((2 * self.t, 4), dtype=np.uint64), np.zeros(18, dtype=np.uint64)
        e._pq_check(e._lib.kzg_circuit_open_blinded_device(e._h, self._c, C.c_void_p(d_wires), self.n if stride is None else stride,
                                                           C.c_void_p(d_z), C.c_void_p(d_public_inputs), C.c_void_p(d_t_coeffs),
                                                           _ptr(ch[0]), _ptr(ch[1]), _ptr(ch[2]), _ptr(ch[3]), _ptr(ch[4]), _ptr(b),
                                                           _ptr(ev), _ptr(p1)))
        return self._split_evals(ev), G1Point(p1)

    # -- the lookup argument of a circuit with a table --
    def lookup_columns(self, wires, theta, beta, n=None, engine=None):
        """kzg_circuit_lookup_columns: wires as quotient() takes them -> (f, T, m, phi) as (n, 4) arrays and phi_n as a Scalar.
        KzgError(KZG_ERR_INVALID_ARG) carries .bad_row for a tuple outside the table or a zero denominator"""
        e = self._eng if engine is None else engine
        a, t, stride, n = e._columns(wires, self.n if n is None else n)
        assert t == self.t and n == self.n
        th, bl = theta.limbs(), beta.limbs()
        f, tb, m, phi = (np.zeros((n, 4), dtype=np.uint64) for _ in range(4))
        last = np.zeros(4, dtype=np.uint64)
        bad = C.c_size_t(0)
        try:
            e._pq_check(e._lib.kzg_circuit_lookup_columns(e._h, self._c, _ptr(a), stride, _ptr(th), _ptr(bl), _ptr(f), _ptr(tb), _ptr(m),
                                                          _ptr(phi), _ptr(last), C.byref(bad)))
        except KzgError as err:
            err.bad_row = None if bad.value == C.c_size_t(-1).value else int(bad.value)
            raise
        return f, tb, m, phi, Scalar.from_limbs(last)

    def lookup_quotient(self, wires, z, mult, phi, alpha, beta, gamma, theta, public_inputs=None, n=None, want_coeffs=True,
                        want_commitments=True, engine=None):
        """kzg_circuit_lookup_quotient: quotient() without a gate, with the lookup's term made from mult and phi (the (n, 4) arrays
        of lookup_columns) -> as quotient()"""
        e = self._eng if engine is None else engine
        a, t, stride, n = e._columns(wires, self.n if n is None else n)
        assert t == self.t and n == self.n
        zz, mm, pp = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4) for x in (z, mult, phi))
        assert zz.shape[0] >= n and mm.shape[0] >= n and pp.shape[0] >= n
        N = n << self.log_ext
        pi = None if public_inputs is None else np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1, 4)
        assert pi is None or pi.shape[0] >= n
        al, bl, gl, th = alpha.limbs(), beta.limbs(), gamma.limbs(), theta.limbs()
        coeffs = np.zeros((N - n, 4), dtype=np.uint64) if want_coeffs else None
        p1s = np.zeros(((1 << self.log_ext) - 1, 18), dtype=np.uint64) if want_commitments else None
        e._pq_check(e._lib.kzg_circuit_lookup_quotient(e._h, self._c, _ptr(a), stride, _ptr(zz), _ptr(mm), _ptr(pp),
                                                       None if pi is None else _ptr(pi), _ptr(al), _ptr(bl), _ptr(gl), _ptr(th),
                                                       None if coeffs is None else _ptr(coeffs), None if p1s is None else _ptr(p1s)))
        return coeffs, None if p1s is None else [G1Point(p) for p in p1s]

    def lookup_quotient_blinded(self, wires, z, mult, phi, alpha, beta, gamma, theta, blinders, public_inputs=None, n=None,
                                want_coeffs=True, want_commitments=True, engine=None):
        """kzg_circuit_lookup_quotient_blinded: lookup_quotient() for the blinded columns, blinders the (2 t + e + 6, 4) array of
        circuit_lookup_blinders() -> (T~'s (L_T, 4) coefficients or None, the commitments of its e - 1 blinded chunks or None)"""
        e = self._eng if engine is None else engine
        a, t, stride, n = e._columns(wires, self.n if n is None else n)
        assert t == self.t and n == self.n
        zz, mm, pp = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4) for x in (z, mult, phi))
        assert zz.shape[0] >= n and mm.shape[0] >= n and pp.shape[0] >= n
        pi = None if public_inputs is None else np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1, 4)
        assert pi is None or pi.shape[0] >= n
        b = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1, 4)
        ext = 1 << self.log_ext
        assert b.shape[0] == 2 * t + ext + 6
        al, bl, gl, th = alpha.limbs(), beta.limbs(), gamma.limbs(), theta.limbs()
        coeffs = np.zeros(((ext - 1) * n + t + 3, 4), dtype=np.uint64) if want_coeffs else None
        p1s = np.zeros((ext - 1, 18), dtype=np.uint64) if want_commitments else None
        e._pq_check(e._lib.kzg_circuit_lookup_quotient_blinded(e._h, self._c, _ptr(a), stride, _ptr(zz), _ptr(mm), _ptr(pp),
                                                               None if pi is None else _ptr(pi), _ptr(al), _ptr(bl), _ptr(gl), _ptr(th),
                                                               _ptr(b), None if coeffs is None else _ptr(coeffs),
                                                               None if p1s is None else _ptr(p1s)))
        return coeffs, None if p1s is None else [G1Point(p) for p in p1s]

    def _lookup_prove(self, fn, e, wires_arg, stride, public_inputs, blinders=None):
        assert self.key is not None and len(self.key) == 2 * self.t + self.c + 3, "lookup_prove: the key of circuit_create_lookup"
        rows = np.ascontiguousarray(np.stack([c.p1 for c in self.key]), dtype=np.uint64)
        pub = None if public_inputs is None else np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(circuit_lookup_proof_size(self.t, self.log_ext, self.c), dtype=np.uint8)
        bad = C.c_size_t(0)
        more = ()
        if blinders is not None:
            bl = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1, 4)
            assert bl.shape[0] == 2 * self.t + (1 << self.log_ext) + 6
            more = (_ptr(bl),)
        try:
            e._pq_check(fn(e._h, self._c, _ptr(rows), wires_arg, stride, None if pub is None else _ptr(pub),
                           0 if pub is None else pub.shape[0], *more, _ptr(out), C.byref(bad)))
        except KzgError as err:
            err.bad_row = None if bad.value == C.c_size_t(-1).value else int(bad.value)
            raise
        return out.tobytes()

    def lookup_prove(self, wires, public_inputs=None, n=None, engine=None):
        """kzg_circuit_lookup_prove: wires a (t, stride, 4) array, public_inputs None or the (n_public, 4) values of rows
        [0, n_public) -> the proof bytes (circuit_lookup_proof_size of them); NOT zero-knowledge.  A KzgError carries .bad_row"""
        e = self._eng if engine is None else engine
        a, t, stride, n = e._columns(wires, self.n if n is None else n)
        assert t == self.t and n == self.n
        return self._lookup_prove(e._lib.kzg_circuit_lookup_prove, e, _ptr(a), stride, public_inputs)

    def lookup_prove_device(self, d_wires, public_inputs=None, stride=None):
        """kzg_circuit_lookup_prove_device: the wires in a device buffer of the circuit's (single-device) context"""
        e = self._eng
        return self._lookup_prove(e._lib.kzg_circuit_lookup_prove_device, e, C.c_void_p(d_wires), self.n if stride is None else stride,
                                  public_inputs)

    def lookup_prove_blinded(self, wires, blinders, public_inputs=None, n=None, engine=None):
        """kzg_circuit_lookup_prove_blinded: lookup_prove() with the (2 t + e + 6, 4) array of circuit_lookup_blinders() -> the
        proof bytes, same format and verifier; zero-knowledge.  A KzgError carries .bad_row"""
        e = self._eng if engine is None else engine
        a, t, stride, n = e._columns(wires, self.n if n is None else n)
        assert t == self.t and n == self.n
        return self._lookup_prove(e._lib.kzg_circuit_lookup_prove_blinded, e, _ptr(a), stride, public_inputs, blinders)

    def lookup_prove_blinded_device(self, d_wires, blinders, public_inputs=None, stride=None):
        """kzg_circuit_lookup_prove_blinded_device: the wires in a device buffer of the circuit's (single-device) context"""
        e = self._eng
        return self._lookup_prove(e._lib.kzg_circuit_lookup_prove_blinded_device, e, C.c_void_p(d_wires),
                                  self.n if stride is None else stride, public_inputs, blinders)

    # -- custom gates: selector x wire-monomial terms --
    def custom_gate(self, wires, n=None, engine=None):
        """kzg_circuit_custom_gate (test hook, no SRS): wires a (t, stride, 4) array -> the (N, 4) values of
        G' = sum_s qx_s prod_j f_j^p[s][j] on the coset"""
        e = self._eng if engine is None else engine
        a, t, stride, n = e._columns(wires, self.n if n is None else n)
        assert t == self.t and n == self.n
        out = np.zeros((n << self.log_ext, 4), dtype=np.uint64)
        e._pq_check(e._lib.kzg_circuit_custom_gate(e._h, self._c, _ptr(a), stride, _ptr(out)))
        return out

    def custom_quotient(self, wires, z, alpha, beta, gamma, blinders=None, public_inputs=None, n=None, want_coeffs=True,
                        want_commitments=True, engine=None):
        """kzg_circuit_custom_quotient: quotient() without a gate (blinders None) or quotient_blinded(), with the custom terms made
        from the wires on the device -> as those return"""
        e = self._eng if engine is None else engine
        a, t, stride, n = e._columns(wires, self.n if n is None else n)
        assert t == self.t and n == self.n
        zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 4)
        pi = None if public_inputs is None else np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1, 4)
        assert zz.shape[0] >= n and (pi is None or pi.shape[0] >= n)
        ext = 1 << self.log_ext
        b = None if blinders is None else np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1, 4)
        assert b is None or b.shape[0] == 2 * t + 3 + ext - 2
        al, bl, gl = alpha.limbs(), beta.limbs(), gamma.limbs()
        rows = (ext - 1) * n + (0 if b is None else t + 3)
        coeffs = np.zeros((rows, 4), dtype=np.uint64) if want_coeffs else None
        p1s = np.zeros((ext - 1, 18), dtype=np.uint64) if want_commitments else None
        e._pq_check(e._lib.kzg_circuit_custom_quotient(e._h, self._c, _ptr(a), stride, _ptr(zz), None if pi is None else _ptr(pi),
                                                       _ptr(al), _ptr(bl), _ptr(gl), None if b is None else _ptr(b),
                                                       None if coeffs is None else _ptr(coeffs), None if p1s is None else _ptr(p1s)))
        return coeffs, None if p1s is None else [G1Point(p) for p in p1s]

    def custom_prove(self, wires, public_inputs=None, blinders=None, n=None, engine=None):
        """kzg_circuit_custom_prove: prove()'s arguments on a circuit of circuit_create_custom -> the proof bytes
        (circuit_proof_size of them) of the statement with the custom terms"""
        e = self._eng if engine is None else engine
        a, t, stride, n = e._columns(wires, self.n if n is None else n)
        assert t == self.t and n == self.n
        return self._prove(e._lib.kzg_circuit_custom_prove, e, _ptr(a), stride, public_inputs, blinders)

    def custom_prove_device(self, d_wires, public_inputs=None, blinders=None, stride=None):
        """kzg_circuit_custom_prove_device: the wires in a device buffer of the circuit's (single-device) context"""
        e = self._eng
        return self._prove(e._lib.kzg_circuit_custom_prove_device, e, C.c_void_p(d_wires), self.n if stride is None else stride,
                           public_inputs, blinders)

    # -- custom gates that read the next row --
    def custom_next_gate(self, wires, n=None, engine=None):
        """kzg_circuit_custom_next_gate (test hook, no SRS): wires a (t, stride, 4) array -> the (N, 4) values of
        G' = sum_s qx_s prod_j f_j(X)^p[s][j] f_j(w X)^p'[s][j] on the coset"""
        e = self._eng if engine is None else engine
        a, t, stride, n = e._columns(wires, self.n if n is None else n)
        assert t == self.t and n == self.n
        out = np.zeros((n << self.log_ext, 4), dtype=np.uint64)
        e._pq_check(e._lib.kzg_circuit_custom_next_gate(e._h, self._c, _ptr(a), stride, _ptr(out)))
        return out

    def custom_next_quotient(self, wires, z, alpha, beta, gamma, public_inputs=None, n=None, want_coeffs=True, want_commitments=True,
                             engine=None):
        """kzg_circuit_custom_next_quotient: quotient() without a gate, with the next-row terms made from the wires on the
        device -> as it returns"""
        e = self._eng if engine is None else engine
        a, t, stride, n = e._columns(wires, self.n if n is None else n)
        assert t == self.t and n == self.n
        zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 4)
        pi = None if public_inputs is None else np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1, 4)
        assert zz.shape[0] >= n and (pi is None or pi.shape[0] >= n)
        ext = 1 << self.log_ext
        al, bl, gl = alpha.limbs(), beta.limbs(), gamma.limbs()
        coeffs = np.zeros(((ext - 1) * n, 4), dtype=np.uint64) if want_coeffs else None
        p1s = np.zeros((ext - 1, 18), dtype=np.uint64) if want_commitments else None
        e._pq_check(e._lib.kzg_circuit_custom_next_quotient(e._h, self._c, _ptr(a), stride, _ptr(zz), None if pi is None else _ptr(pi),
                                                            _ptr(al), _ptr(bl), _ptr(gl), None if coeffs is None else _ptr(coeffs),
                                                            None if p1s is None else _ptr(p1s)))
        return coeffs, None if p1s is None else [G1Point(p) for p in p1s]

    def _next_proof_size(self):
        return 48 * (self.t + (1 << self.log_ext) + 1) + 32 * (2 * self.t + max(self.rho, 1))

    def custom_next_prove(self, wires, public_inputs=None, blinders=None, n=None, engine=None):
        """kzg_circuit_custom_next_prove: prove()'s arguments on a circuit of circuit_create_custom_next -> the proof bytes
        (circuit_custom_next_proof_size of them).  Next-row proofs are plain: blinders other than None are refused"""
        e = self._eng if engine is None else engine
        a, t, stride, n = e._columns(wires, self.n if n is None else n)
        assert t == self.t and n == self.n
        return self._prove(e._lib.kzg_circuit_custom_next_prove, e, _ptr(a), stride, public_inputs, blinders, self._next_proof_size())

    def custom_next_prove_device(self, d_wires, public_inputs=None, blinders=None, stride=None):
        """kzg_circuit_custom_next_prove_device: the wires in a device buffer of the circuit's (single-device) context"""
        e = self._eng
        return self._prove(e._lib.kzg_circuit_custom_next_prove_device, e, C.c_void_p(d_wires), self.n if stride is None else stride,
                           public_inputs, blinders, self._next_proof_size())

    def column_device(self, which, form):
        """kzg_circuit_column_device: (device pointer, length) of a resident column, read-only"""
        e = self._eng
        p, ln = C.c_void_p(), C.c_size_t(0)
        e._pq_check(e._lib.kzg_circuit_column_device(e._h, self._c, which, form, C.byref(p), C.byref(ln)))
        return p.value, int(ln.value)


class SetupArtifactsGenerator:
    def __init__(self, secret_be, device=0):
        assert len(secret_be) == 32
        self.secret = bytes(secret_be)
        self.device = device

    def take(self, n, engine=None):
        eng = engine or Engine(self.device)
        eng.srs_generate(self.secret, n)
        return eng


def domain_root(log_n):
    """w_n for n = 2^log_n: 7^((r - 1) / n) mod r, as a Scalar (host only)"""
    out = np.zeros(4, dtype=np.uint64)
    _check(load_library().kzg_domain_root(log_n, _ptr(out)))
    return Scalar.from_limbs(out)


def srs_g2_at(secret_be, index=1):
    """kzg_srs_g2_at: the G2 half of SetupArtifact `index`, [s^index]G2, as a blst_p2 (36 x uint64) -- what
    Evaluation::verify_proof reads from setup_artifacts[1] (src/polynomial.rs:284)."""
    lib = load_library()
    out = np.zeros(36, dtype=np.uint64)
    _check(lib.kzg_srs_g2_at(bytes(secret_be), int(index), _ptr(out)))
    return out


def g2_mul(p2, scalar_be):
    """kzg_g2_mul: [k]Q on the host for a blst_p2 (36 x uint64) and 32 big-endian bytes (reduced mod r), normalised"""
    assert len(scalar_be) == 32
    q = np.ascontiguousarray(p2, dtype=np.uint64).reshape(36)
    out = np.zeros(36, dtype=np.uint64)
    _check(load_library().kzg_g2_mul(_ptr(q), bytes(scalar_be), _ptr(out)))
    return out


def verify_srs_update(before, after, tau_g2):
    """kzg_srs_verify_update: e(after, [1]G2) == e(before, tau_g2) -- one link of a ceremony transcript; before, after:
    G1Points (SRS[1] around a contribution), tau_g2 = [tau]G2 as a blst_p2"""
    q = np.ascontiguousarray(tau_g2, dtype=np.uint64).reshape(36)
    ok = C.c_int(0)
    _check(load_library().kzg_srs_verify_update(_ptr(before.p1), _ptr(after.p1), _ptr(q), C.byref(ok)))
    return bool(ok.value)


def sha256(data, piece=None, path=KZG_SHA256_AUTO):
    """kzg_sha256: the library's SHA-256 of `data` (bytes).  piece / path: feed the streaming interface that many bytes at a
    time on the path asked for (kzg_sha256_pieces; KZG_SHA256_SHANI raises KzgError on a CPU without the extensions)"""
    lib = load_library()
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.zeros(32, dtype=np.uint8)
    src = _ptr(a) if a.size else None
    if piece is None and path == KZG_SHA256_AUTO:
        _check(lib.kzg_sha256(src, a.size, _ptr(out)))
    else:
        _check(lib.kzg_sha256_pieces(src, a.size, piece or max(a.size, 1), path, _ptr(out)))
    return out.tobytes()


def sha256_has_shani():
    """whether the library's SHA-256 runs on the CPU's SHA extensions"""
    return bool(load_library().kzg_sha256_has_shani())


def blob_challenges_bytes(blobs_be, n, commitments48, stride=None):
    """kzg_blob_challenges_bytes: the Fiat-Shamir challenge of every blob (batch x stride x 32 bytes, the first n values of a
    stride being the blob) with its commitment (batch x 48 bytes, hashed as given) -> batch x 32 big-endian bytes, each < r"""
    lib = load_library()
    a = np.frombuffer(bytes(blobs_be), dtype=np.uint8) if not isinstance(blobs_be, np.ndarray) else np.ascontiguousarray(blobs_be, dtype=np.uint8).reshape(-1)
    com = np.frombuffer(bytes(commitments48), dtype=np.uint8)
    stride = n if stride is None else stride
    if not (n and stride >= n and a.size % (32 * stride) == 0 and com.size % 48 == 0 and com.size // 48 == a.size // (32 * stride)):
        raise ValueError("whole blobs of n values, `stride` values apart, and one commitment per blob")
    batch = com.size // 48
    out = np.zeros((max(batch, 1), 32), dtype=np.uint8)
    _check(lib.kzg_blob_challenges_bytes(_ptr(a) if a.size else None, n, batch, stride, _ptr(com) if com.size else None, _ptr(out)))
    return out[:batch].tobytes()


def verify_proof(commitment, proof, z, y, s_g2):
    """kzg_verify_proof: e(proof, [s]G2 - [z]G2) == e(commitment - [y]G1, G2) on the host."""
    lib = load_library()
    g2 = np.ascontiguousarray(s_g2, dtype=np.uint64).reshape(36)
    ok = C.c_int(0)
    zl, yl = z.limbs(), y.limbs()
    _check(lib.kzg_verify_proof(_ptr(commitment.p1), _ptr(proof.p1), _ptr(zl), _ptr(yl), _ptr(g2), C.byref(ok)))
    return bool(ok.value)


def verify_proof_batch(commitments, proofs, zs, ys, s_g2):
    """kzg_verify_proof_batch: one verdict per (commitment, proof, z, y), checks spread over the host cores."""
    lib = load_library()
    n = len(commitments)
    assert len(proofs) == n and len(zs) == n and len(ys) == n
    g2 = np.ascontiguousarray(s_g2, dtype=np.uint64).reshape(36)
    cs = np.ascontiguousarray(np.stack([c.p1 for c in commitments]) if n else np.zeros((0, 18)), dtype=np.uint64)
    ps = np.ascontiguousarray(np.stack([p.p1 for p in proofs]) if n else np.zeros((0, 18)), dtype=np.uint64)
    zl = np.ascontiguousarray(np.stack([z.limbs() for z in zs]) if n else np.zeros((0, 4)), dtype=np.uint64)
    yl = np.ascontiguousarray(np.stack([y.limbs() for y in ys]) if n else np.zeros((0, 4)), dtype=np.uint64)
    ok = np.zeros(max(n, 1), dtype=np.int32)
    _check(lib.kzg_verify_proof_batch(_ptr(cs), _ptr(ps), _ptr(zl), _ptr(yl), _ptr(g2), n, _ptr(ok)))
    return [bool(v) for v in ok[:n]]


def _scalar_rows(values):
    """k Scalars -> k x 4 uint64 (blst_fr images, Montgomery), contiguous"""
    return np.ascontiguousarray(np.stack([v.limbs() for v in values]) if len(values) else np.zeros((1, 4)), dtype=np.uint64)


def verify_points(commitment, proof, zs, ys, setup_g1, setup_g2):
    """kzg_verify_points: e(proof, [Z(s)]G2) == e(commitment - [I(s)]G1, G2) on the host.  setup_g1: at least k
    blst_p1 rows ([s^j]G1, j < k); setup_g2: k + 1 blst_p2 rows ([s^j]G2, j <= k), e.g. from srs_g2_at."""
    lib = load_library()
    g1 = np.ascontiguousarray(setup_g1, dtype=np.uint64).reshape(-1, 18)
    g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
    k = len(zs)
    assert len(ys) == k and g1.shape[0] >= k and g2.shape[0] >= k + 1
    ok = C.c_int(0)
    _check(lib.kzg_verify_points(_ptr(commitment.p1), _ptr(proof.p1), _ptr(_scalar_rows(zs)), _ptr(_scalar_rows(ys)), k,
                                 _ptr(g1), 144, _ptr(g2), 288, C.byref(ok)))
    return bool(ok.value)


def _sets_arrays(set_of, sets):
    """(set_of as uint32, the set sizes as uint32, the points set after set as k x 4 uint64)"""
    so = np.ascontiguousarray(list(set_of) if len(set_of) else [0], dtype=np.uint32)
    sl = np.ascontiguousarray([len(s) for s in sets] if len(sets) else [0], dtype=np.uint32)
    return so, sl, _scalar_rows([z for s in sets for z in s])


def _sets_value_count(set_of, sets):
    return max(sum(len(sets[g]) for g in set_of if 0 <= g < len(sets)), 1)


def _sets_split_values(ys, set_of, sets):
    out, at = [], 0
    for g in set_of:
        out.append([Scalar.from_limbs(ys[at + j]) for j in range(len(sets[g]))])
        at += len(sets[g])
    return out


def verify_sets(commitments, set_of, sets, ys, gamma, proof, setup_g1, setup_g2):
    """kzg_verify_sets: prod_g e(A_g, [Z_(T \\ S_g)(s)]G2) == e(proof, [Z_T(s)]G2) on the host.  ys[i]: the values of
    polynomial i on sets[set_of[i]]; setup_g1: at least max |S_g| blst_p1 rows ([s^j]G1); setup_g2: at least |T| + 1 blst_p2
    rows ([s^j]G2, j <= |T|, T the distinct points over all sets), e.g. from srs_g2_at.  gamma has to be the challenge the
    protocol draws AFTER the commitments and the values; nothing is hashed here."""
    lib = load_library()
    t = len(commitments)
    assert len(set_of) == t and len(ys) == t
    g1 = np.ascontiguousarray(setup_g1, dtype=np.uint64).reshape(-1, 18)
    g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
    distinct = len({z.v for s in sets for z in s})
    assert g1.shape[0] >= max(len(s) for s in sets) and g2.shape[0] >= distinct + 1
    cs = np.ascontiguousarray(np.stack([c.p1 for c in commitments]) if t else np.zeros((1, 18)), dtype=np.uint64)
    so, sl, zl = _sets_arrays(set_of, sets)
    yl = _scalar_rows([y for row in ys for y in row])
    ok = C.c_int(0)
    _check(lib.kzg_verify_sets(_ptr(cs), t, _ptr(so), _ptr(sl), len(sets), _ptr(zl), _ptr(yl), _ptr(gamma.limbs()),
                               _ptr(proof.p1), _ptr(g1), 144, _ptr(g2), 288, C.byref(ok)))
    return bool(ok.value)


def ml_verify(commitment, us, v, folds, ys, r, gamma, proof, setup_g1, setup_g2, ell=None):
    """kzg_ml_verify: the fold relation at r for every level, then kzg_verify_sets over [C, C_1 .. C_(ell-1)] on the one set
    {r, -r, r^2}.  ys[i] = [f_i(r), f_i(-r), f_i(r^2)]; setup_g1: at least three blst_p1 rows; setup_g2: [s^j]G2 for j <= 3.
    r has to be drawn after the fold commitments and gamma after the values; nothing is hashed here."""
    lib = load_library()
    ell = len(us) if ell is None else ell
    g1 = np.ascontiguousarray(setup_g1, dtype=np.uint64).reshape(-1, 18)
    g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
    assert g1.shape[0] >= 3 and g2.shape[0] >= 4
    fl = np.ascontiguousarray(np.stack([c.p1 for c in folds]) if len(folds) else np.zeros((1, 18)), dtype=np.uint64)
    yl = _scalar_rows([y for row in ys for y in row])
    ok = C.c_int(0)
    _check(lib.kzg_ml_verify(_ptr(commitment.p1), ell, _ptr(_scalar_rows(us)), _ptr(v.limbs()), _ptr(fl), _ptr(yl), _ptr(r.limbs()),
                             _ptr(gamma.limbs()), _ptr(proof.p1), _ptr(g1), 144, _ptr(g2), 288, C.byref(ok)))
    return bool(ok.value)


def circuit_blinded_sizes(n, t, log_ext):
    """kzg_circuit_blinded_sizes -> (entries of the blinder array, L_T); KzgError(KZG_ERR_INVALID_ARG) for a shape the blinded
    calls refuse (2^log_ext n < t n + t + 4)"""
    lib = load_library()
    nb, lt = C.c_size_t(0), C.c_size_t(0)
    _check(lib.kzg_circuit_blinded_sizes(n, t, log_ext, C.byref(nb), C.byref(lt)))
    return int(nb.value), int(lt.value)


def circuit_blinders(t, log_ext):
    """kzg_circuit_blinders: the blinder array of one proof -- t pairs for the wires, three for z, 2^log_ext - 2 for the chunks of
    T -- as a (count, 4) array of canonical blst_fr drawn from the OS CSPRNG"""
    lib = load_library()
    out = np.zeros((2 * t + 3 + (1 << log_ext) - 2, 4), dtype=np.uint64)
    _check(lib.kzg_circuit_blinders(t, log_ext, _ptr(out)))
    return out


def circuit_lookup_blinded_sizes(n, t, log_ext, c):
    """kzg_circuit_lookup_blinded_sizes -> (entries of the blinder array, 2 t + e + 6; L_T); KzgError(KZG_ERR_INVALID_ARG) for a
    shape the blinded lookup calls refuse (max(t n + t + 3, 3 n + 2) >= 2^log_ext n, or a shape no lookup circuit has)"""
    lib = load_library()
    nb, lt = C.c_size_t(0), C.c_size_t(0)
    _check(lib.kzg_circuit_lookup_blinded_sizes(n, t, log_ext, c, C.byref(nb), C.byref(lt)))
    return int(nb.value), int(lt.value)


def circuit_lookup_blinders(t, log_ext):
    """kzg_circuit_lookup_blinders: the blinder array of one blinded lookup proof -- circuit_blinders' groups, then three for phi
    and two for m -- as a (2 t + e + 6, 4) array of canonical blst_fr drawn from the OS CSPRNG"""
    lib = load_library()
    out = np.zeros((2 * t + (1 << log_ext) + 6, 4), dtype=np.uint64)
    _check(lib.kzg_circuit_lookup_blinders(t, log_ext, _ptr(out)))
    return out


def circuit_verify(key, n, log_ext, shifts, wire_commitments, z_commitment, t_commitments, public_inputs, evals, alpha, beta, gamma,
                   zeta, v, proof, setup_g1, setup_g2):
    """kzg_circuit_verify on the host: key the 2 t + 2 commitments of circuit_create in its order, t_commitments those of T's
    2^log_ext - 1 chunks, public_inputs the values at rows 0 .. len - 1 (Scalars; the later rows are zero), evals what
    Circuit.open returned: (f_j(zeta), sigma_j(zeta), z(zeta w)).  setup_g1: at least one blst_p1 row; setup_g2: at least three
    blst_p2 rows ([s^j]G2, j <= 2).  The challenges have to be the transcript's; nothing is hashed here."""
    lib = load_library()
    t = len(wire_commitments)
    abar, sbar, zw = evals
    assert len(key) == 2 * t + 2 and len(shifts) == t and len(abar) == t and len(sbar) == t - 1
    assert len(t_commitments) == (1 << log_ext) - 1
    g1 = np.ascontiguousarray(setup_g1, dtype=np.uint64).reshape(-1, 18)
    g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
    assert g1.shape[0] >= 1 and g2.shape[0] >= 3
    rows = lambda pts: np.ascontiguousarray(np.stack([c.p1 for c in pts]), dtype=np.uint64)
    pub = list(public_inputs) if public_inputs is not None else []
    ok = C.c_int(0)
    _check(lib.kzg_circuit_verify(_ptr(rows(key)), n, t, log_ext, _ptr(_scalar_rows(shifts)), _ptr(rows(wire_commitments)),
                                  _ptr(z_commitment.p1), _ptr(rows(t_commitments)), _ptr(_scalar_rows(pub)) if pub else None, len(pub),
                                  _ptr(_scalar_rows(list(abar) + list(sbar) + [zw])), _ptr(alpha.limbs()), _ptr(beta.limbs()),
                                  _ptr(gamma.limbs()), _ptr(zeta.limbs()), _ptr(v.limbs()), _ptr(proof.p1), _ptr(g1), 144, _ptr(g2),
                                  288, C.byref(ok)))
    return bool(ok.value)


def circuit_proof_size(t, log_ext):
    """kzg_circuit_proof_size: the bytes of a proof of a circuit with t wires, 48 (t + 2^log_ext + 1) + 64 t"""
    out = C.c_size_t(0)
    _check(load_library().kzg_circuit_proof_size(t, log_ext, C.byref(out)))
    return out.value


def _proof_statement(key, shifts, public_inputs, proof):
    t = len(shifts)
    assert len(key) == 2 * t + 2
    rows = np.ascontiguousarray(np.stack([c.p1 for c in key]), dtype=np.uint64)
    pub = list(public_inputs) if public_inputs is not None else []
    buf = np.frombuffer(bytes(proof), dtype=np.uint8)
    return t, rows, _scalar_rows(shifts), (_scalar_rows(pub) if pub else None), len(pub), buf


def circuit_proof_challenges(key, n, log_ext, shifts, public_inputs, proof):
    """kzg_circuit_proof_challenges: (beta, gamma, alpha, zeta, v) of the hashed transcript from complete proof bytes.  key,
    shifts and public_inputs as for circuit_verify; nothing is decoded."""
    t, rows, ks, pub, n_public, buf = _proof_statement(key, shifts, public_inputs, proof)
    out = np.zeros((5, 4), dtype=np.uint64)
    _check(load_library().kzg_circuit_proof_challenges(_ptr(rows), n, t, log_ext, _ptr(ks), _ptr(pub) if pub is not None else None,
                                                       n_public, _ptr(buf), buf.shape[0], _ptr(out)))
    return tuple(Scalar.from_limbs(out[i]) for i in range(5))


def circuit_verify_proof(key, n, log_ext, shifts, public_inputs, proof, setup_g1, setup_g2):
    """kzg_circuit_verify_proof on the host: decodes the proof bytes, derives the challenges, runs circuit_verify.  False also
    for bytes that do not decode (points are checked to lie on the curve, not in the subgroup)."""
    t, rows, ks, pub, n_public, buf = _proof_statement(key, shifts, public_inputs, proof)
    g1 = np.ascontiguousarray(setup_g1, dtype=np.uint64).reshape(-1, 18)
    g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
    assert g1.shape[0] >= 1 and g2.shape[0] >= 3
    ok = C.c_int(0)
    _check(load_library().kzg_circuit_verify_proof(_ptr(rows), n, t, log_ext, _ptr(ks), _ptr(pub) if pub is not None else None, n_public,
                                                   _ptr(buf), buf.shape[0], _ptr(g1), 144, _ptr(g2), 288, C.byref(ok)))
    return bool(ok.value)


def circuit_custom_blinded_sizes(n, t, log_ext, d_max):
    """kzg_circuit_custom_blinded_sizes -> (entries of the blinder array, L_T); KzgError(KZG_ERR_INVALID_ARG) for a shape the
    blinded calls refuse with custom gates of degree d_max: max(t n + t + 3, d_max (n + 1)) has to be <= L_T and < 2^log_ext n"""
    nb, lt = C.c_size_t(0), C.c_size_t(0)
    _check(load_library().kzg_circuit_custom_blinded_sizes(n, t, log_ext, d_max, C.byref(nb), C.byref(lt)))
    return int(nb.value), int(lt.value)


def _custom_proof_statement(key, exponents, shifts, public_inputs, proof):
    t = len(shifts)
    ex = np.ascontiguousarray(exponents, dtype=np.uint8).reshape(-1, t)
    assert len(key) == 2 * t + 2 + ex.shape[0]
    rows = np.ascontiguousarray(np.stack([k.p1 for k in key]), dtype=np.uint64)
    pub = list(public_inputs) if public_inputs is not None else []
    buf = np.frombuffer(bytes(proof), dtype=np.uint8)
    return t, ex, rows, _scalar_rows(shifts), (_scalar_rows(pub) if pub else None), len(pub), buf


def circuit_custom_proof_challenges(key, n, log_ext, exponents, shifts, public_inputs, proof):
    """kzg_circuit_custom_proof_challenges: (beta, gamma, alpha, zeta, v) of the hashed transcript from complete proof bytes.
    key: the 2 t + 2 + g commitments of circuit_create_custom, exponents its (g, t) bytes; nothing is decoded."""
    t, ex, rows, ks, pub, n_public, buf = _custom_proof_statement(key, exponents, shifts, public_inputs, proof)
    out = np.zeros((5, 4), dtype=np.uint64)
    _check(load_library().kzg_circuit_custom_proof_challenges(_ptr(rows), n, t, log_ext, ex.shape[0], _ptr(ex), _ptr(ks),
                                                              _ptr(pub) if pub is not None else None, n_public, _ptr(buf), buf.shape[0],
                                                              _ptr(out)))
    return tuple(Scalar.from_limbs(out[i]) for i in range(5))


def circuit_custom_verify_proof(key, n, log_ext, exponents, shifts, public_inputs, proof, setup_g1, setup_g2):
    """kzg_circuit_custom_verify_proof on the host: decodes the proof bytes, derives the challenges, forms [r_X], checks the
    opening; plain and blinded proofs alike.  False also for bytes that do not decode."""
    t, ex, rows, ks, pub, n_public, buf = _custom_proof_statement(key, exponents, shifts, public_inputs, proof)
    g1 = np.ascontiguousarray(setup_g1, dtype=np.uint64).reshape(-1, 18)
    g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
    assert g1.shape[0] >= 1 and g2.shape[0] >= 3
    ok = C.c_int(0)
    _check(load_library().kzg_circuit_custom_verify_proof(_ptr(rows), n, t, log_ext, ex.shape[0], _ptr(ex), _ptr(ks),
                                                          _ptr(pub) if pub is not None else None, n_public, _ptr(buf), buf.shape[0],
                                                          _ptr(g1), 144, _ptr(g2), 288, C.byref(ok)))
    return bool(ok.value)


def circuit_custom_next_proof_size(t, log_ext, rho):
    """kzg_circuit_custom_next_proof_size: the bytes of a next-row proof, 48 (t + 2^log_ext + 1) + 32 (2 t + rho)"""
    out = C.c_size_t(0)
    _check(load_library().kzg_circuit_custom_next_proof_size(t, log_ext, rho, C.byref(out)))
    return out.value


def _next_exponents(exponents_next, ex):
    exn = np.ascontiguousarray(exponents_next, dtype=np.uint8).reshape(-1, ex.shape[1])
    assert exn.shape == ex.shape
    return exn


def circuit_custom_next_proof_challenges(key, n, log_ext, exponents, exponents_next, shifts, public_inputs, proof):
    """kzg_circuit_custom_next_proof_challenges: (beta, gamma, alpha, zeta, v) of the hashed transcript from complete proof bytes.
    key: the 2 t + 2 + g commitments of circuit_create_custom_next, exponents and exponents_next its (g, t) bytes."""
    t, ex, rows, ks, pub, n_public, buf = _custom_proof_statement(key, exponents, shifts, public_inputs, proof)
    exn = _next_exponents(exponents_next, ex)
    out = np.zeros((5, 4), dtype=np.uint64)
    _check(load_library().kzg_circuit_custom_next_proof_challenges(_ptr(rows), n, t, log_ext, ex.shape[0], _ptr(ex), _ptr(exn), _ptr(ks),
                                                                   _ptr(pub) if pub is not None else None, n_public, _ptr(buf),
                                                                   buf.shape[0], _ptr(out)))
    return tuple(Scalar.from_limbs(out[i]) for i in range(5))


def circuit_custom_next_verify_proof(key, n, log_ext, exponents, exponents_next, shifts, public_inputs, proof, setup_g1, setup_g2):
    """kzg_circuit_custom_next_verify_proof on the host: decodes the proof bytes, derives the challenges, forms [r_N], checks the
    opening on the three sets.  False also for bytes that do not decode.  setup_g1: [s^j]G1 for j < 2 (the set {zeta, zeta w} has an
    interpolant of degree 1), setup_g2: [s^j]G2 for j <= 2."""
    t, ex, rows, ks, pub, n_public, buf = _custom_proof_statement(key, exponents, shifts, public_inputs, proof)
    exn = _next_exponents(exponents_next, ex)
    g1 = np.ascontiguousarray(setup_g1, dtype=np.uint64).reshape(-1, 18)
    g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
    assert g1.shape[0] >= 2 and g2.shape[0] >= 3
    ok = C.c_int(0)
    _check(load_library().kzg_circuit_custom_next_verify_proof(_ptr(rows), n, t, log_ext, ex.shape[0], _ptr(ex), _ptr(exn), _ptr(ks),
                                                               _ptr(pub) if pub is not None else None, n_public, _ptr(buf),
                                                               buf.shape[0], _ptr(g1), 144, _ptr(g2), 288, C.byref(ok)))
    return bool(ok.value)


def circuit_lookup_proof_size(t, log_ext, c):
    """kzg_circuit_lookup_proof_size: the bytes of a lookup proof, 48 (t + 2^log_ext + 3) + 32 (2 t + c + 2)"""
    out = C.c_size_t(0)
    _check(load_library().kzg_circuit_lookup_proof_size(t, log_ext, c, C.byref(out)))
    return out.value


def _lookup_proof_statement(key, c, shifts, public_inputs, proof):
    t = len(shifts)
    assert len(key) == 2 * t + c + 3
    rows = np.ascontiguousarray(np.stack([k.p1 for k in key]), dtype=np.uint64)
    pub = list(public_inputs) if public_inputs is not None else []
    buf = np.frombuffer(bytes(proof), dtype=np.uint8)
    return t, rows, _scalar_rows(shifts), (_scalar_rows(pub) if pub else None), len(pub), buf


def circuit_lookup_proof_challenges(key, n, log_ext, c, shifts, public_inputs, proof):
    """kzg_circuit_lookup_proof_challenges: (theta, beta, gamma, alpha, zeta, v) of the hashed transcript from complete proof
    bytes.  key: the 2 t + c + 3 commitments of circuit_create_lookup; nothing is decoded."""
    t, rows, ks, pub, n_public, buf = _lookup_proof_statement(key, c, shifts, public_inputs, proof)
    out = np.zeros((6, 4), dtype=np.uint64)
    _check(load_library().kzg_circuit_lookup_proof_challenges(_ptr(rows), n, t, log_ext, c, _ptr(ks),
                                                              _ptr(pub) if pub is not None else None, n_public, _ptr(buf), buf.shape[0],
                                                              _ptr(out)))
    return tuple(Scalar.from_limbs(out[i]) for i in range(6))


def circuit_lookup_verify_proof(key, n, log_ext, c, shifts, public_inputs, proof, setup_g1, setup_g2):
    """kzg_circuit_lookup_verify_proof on the host: decodes the proof bytes, derives the challenges, forms [r_L], checks the
    opening.  False also for bytes that do not decode (points are checked to lie on the curve, not in the subgroup)."""
    t, rows, ks, pub, n_public, buf = _lookup_proof_statement(key, c, shifts, public_inputs, proof)
    g1 = np.ascontiguousarray(setup_g1, dtype=np.uint64).reshape(-1, 18)
    g2 = np.ascontiguousarray(setup_g2, dtype=np.uint64).reshape(-1, 36)
    assert g1.shape[0] >= 1 and g2.shape[0] >= 3
    ok = C.c_int(0)
    _check(load_library().kzg_circuit_lookup_verify_proof(_ptr(rows), n, t, log_ext, c, _ptr(ks), _ptr(pub) if pub is not None else None,
                                                          n_public, _ptr(buf), buf.shape[0], _ptr(g1), 144, _ptr(g2), 288, C.byref(ok)))
    return bool(ok.value)


# ---------------------------------------------------------------------------------------------
# Polynomial / Evaluation: reference src/polynomial.rs
# ---------------------------------------------------------------------------------------------
def combine_claims(commitments, ys, gamma):
    """kzg_combine_claims: (sum gamma^i C_i, sum gamma^i y_i) on the host -- one (commitment, value) pair that any of the
    verifiers takes together with the combined proof.  gamma has to be the challenge the protocol draws AFTER the
    commitments and the values; nothing is hashed here."""
    lib = load_library()
    t = len(commitments)
    assert len(ys) == t
    cs = np.ascontiguousarray(np.stack([c.p1 for c in commitments]) if t else np.zeros((1, 18)), dtype=np.uint64)
    yl, gl = _scalar_rows(ys), gamma.limbs()
    out_c, out_y = np.zeros(18, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    _check(lib.kzg_combine_claims(_ptr(cs), _ptr(yl), t, _ptr(gl), _ptr(out_c), _ptr(out_y)))
    return G1Point(out_c), Scalar.from_limbs(out_y)


def verify_combined(commitments, ys, z, gamma, proof, s_g2):
    """kzg_verify_combined: combine_claims, then verify_proof of the pair at z"""
    lib = load_library()
    t = len(commitments)
    assert len(ys) == t
    g2 = np.ascontiguousarray(s_g2, dtype=np.uint64).reshape(36)
    cs = np.ascontiguousarray(np.stack([c.p1 for c in commitments]) if t else np.zeros((1, 18)), dtype=np.uint64)
    yl, zl, gl = _scalar_rows(ys), z.limbs(), gamma.limbs()
    ok = C.c_int(0)
    _check(lib.kzg_verify_combined(_ptr(cs), _ptr(yl), t, _ptr(zl), _ptr(gl), _ptr(proof.p1), _ptr(g2), C.byref(ok)))
    return bool(ok.value)


class Polynomial:
    def __init__(self, limbs):
        self.limbs = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, 4)

    @staticmethod
    def try_from(values):
        """TryFrom<Vec<i128>> / TryFrom<Vec<Scalar>> (src/polynomial.rs:14-76): trailing zeros are
        dropped, index 0 is kept."""
        if len(values) > 0xFFFFFFFF:
            raise KzgError(KZG_ERR_INVALID_ARG,
                           "Too many coefficients for polynomial, only 2**32 - 1 coefficients is supported. Got %d"
                           % len(values))
        ints = [v.v if isinstance(v, Scalar) else Scalar.from_i128(v).v for v in values]
        last = 0
        for i, v in enumerate(ints):
            if v != 0:
                last = i
        ints = ints[: last + 1] if ints else []
        return Polynomial(scalars_to_limbs(ints))

    @staticmethod
    def from_limbs(limbs):
        """Takes blst_fr rows as they are (applies the same truncation)."""
        a = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, 4)
        nz = np.flatnonzero(a.any(axis=1))
        last = int(nz[-1]) if nz.size else 0
        return Polynomial(a[: last + 1] if a.shape[0] else a)

    @staticmethod
    def from_evaluations(evals, setup):
        """The polynomial whose values over the domain of size n = len(evals) (a power of two) are evals, in natural
        order: evals[i] = P(w_n^i) (domain_root).  Interpolated on the device (setup: an Engine)."""
        return Polynomial.from_limbs(setup.intt_limbs(evals))

    def degree(self):  # src/polynomial.rs:93-98
        return 0 if self.limbs.shape[0] == 0 else self.limbs.shape[0] - 1

    def coefficients(self):
        return [Scalar(v) for v in limbs_to_scalars(self.limbs)]

    def commit(self, setup):  # src/polynomial.rs:200-215
        return setup.commit_limbs(self.limbs)

    def evaluate(self, x, setup):  # src/polynomial.rs:112-123
        return Evaluation(x, setup.evaluate_limbs(self.limbs, x))

    def divide_by_root_minus(self, root, y, setup):
        """(self - y).divide_by_root(root): src/polynomial.rs:128-195."""
        return Polynomial(setup.quotient_limbs(self.limbs, root, y))


class Evaluation:
    def __init__(self, point, result):
        self.point, self.result = point, result

    def generate_proof(self, polynomial, setup):  # src/polynomial.rs:260-269
        return setup.open_limbs(polynomial.limbs, self.point, self.result)

    def verify_proof(self, proof, commitment, s_g2):  # src/polynomial.rs:276-294
        """s_g2: setup_artifacts[1].g2 as 36 x u64 (blst_p2).  Host-side pairing check of the library."""
        return verify_proof(commitment, proof, self.point, self.result, s_g2)
