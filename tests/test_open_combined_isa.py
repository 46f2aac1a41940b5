"""The kernels of the combined openings (combine_kernels.hip: k_combine_eval, k_combine_eval_finish) use no scratch memory and
spill no register: checked in the compiler's metadata for gfx950.  CPU only (hipcc cross-compiles); the assembly comes from
tests/isa_cache.py."""
from isa_cache import kernel_meta, requires_hipcc


@requires_hipcc
def test_combine_kernels_use_no_scratch():
    meta = kernel_meta("combine_kernels.hip")
    combine = {k: v for k, v in meta.items() if "k_combine_eval" in k}
    assert len(combine) == 2, sorted(meta)
    for name, m in combine.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
