"""The batch-verification kernels (verify_kernels.hip) use no scratch and spill no registers; the Fr kernels also stay within 160
VGPRs.  The ladder kernels are latency-bound like the G1 DFT stages and take the registers they need.  Checked in the
compiler's metadata for gfx950.  CPU only (hipcc
cross-compiles); the assembly comes from tests/isa_cache.py."""
from isa_cache import kernel_meta, requires_hipcc


@requires_hipcc
def test_verify_kernels_use_no_scratch():
    meta = kernel_meta("verify_kernels.hip")
    rec = {k: v for k, v in meta.items() if "k_vc_" in k}
    assert len(rec) == 5, sorted(meta)
    for name, m in rec.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        if "_fr_" in name:
            assert m["vgpr_count"] <= 160, (name, m)
