"""The kernels of the multilinear openings (multilinear_kernels.hip: k_ml_fold, k_ml_eval, k_ml_eval_finish, k_ml_combine) are each
present exactly once, use no scratch memory and spill no register: checked in the compiler's resource metadata for gfx950.  The
VGPR and LDS figures are printed, nothing else is inspected.  CPU only (hipcc cross-compiles); the assembly comes from
tests/isa_cache.py."""
from isa_cache import kernel_meta, requires_hipcc

UNIT = "multilinear_kernels.hip"
KERNELS = ("k_ml_foldE", "k_ml_evalE", "k_ml_eval_finishE", "k_ml_combineE")  # ("E": the end of the mangled name)


@requires_hipcc
def test_multilinear_kernels_are_listed_once_and_use_no_scratch():
    meta = kernel_meta(UNIT)
    assert len(meta) == len(KERNELS), sorted(meta)
    for want in KERNELS:
        found = [k for k in meta if want in k]
        assert len(found) == 1, (want, sorted(meta))
        m = meta[found[0]]
        print(found[0], "vgprs", m["vgpr_count"], "lds bytes", m["group_segment_fixed_size"])
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
