"""The recovery kernels (recover_kernels.hip) use no scratch, spill no registers and stay within 160 VGPRs, so that they can
run on one slot beside another slot's accumulation kernel: checked in the compiler's metadata for gfx950.  CPU only (hipcc
cross-compiles); the assembly comes from tests/isa_cache.py."""
from isa_cache import kernel_meta, requires_hipcc


@requires_hipcc
def test_recover_kernels_fit_beside_accumulation():
    meta = kernel_meta("recover_kernels.hip")
    rec = {k: v for k, v in meta.items() if "k_rec_" in k}
    assert len(rec) == 7, sorted(meta)
    for name, m in rec.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 160, (name, m)
