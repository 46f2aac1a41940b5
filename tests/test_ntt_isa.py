"""The NTT pass kernel (ntt_kernels.hip: k_ntt_pass) uses no scratch memory and spills nothing: checked in the compiler's
metadata for gfx950.  CPU only (hipcc cross-compiles); the assembly comes from tests/isa_cache.py."""
from isa_cache import kernel_meta, requires_hipcc


@requires_hipcc
def test_ntt_kernel_uses_no_scratch():
    meta = kernel_meta("ntt_kernels.hip")
    ntt = {k: v for k, v in meta.items() if "k_ntt_pass" in k}
    assert len(ntt) == 1, sorted(meta)
    for name, m in ntt.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)  # two 256-thread workgroups per CU need at most 128
