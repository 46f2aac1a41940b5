"""The barycentric-evaluation kernels (bary_kernels.hip) use no scratch and spill no registers, and stay within the 160 VGPRs
that leave room beside the accumulation kernel; the counts found are pinned.  Checked in the
compiler's metadata for gfx950.  CPU only (hipcc cross-compiles); the assembly comes from tests/isa_cache.py."""
from isa_cache import kernel_meta

VGPRS = {"k_bary_partial": 132, "k_bary_finish": 44}  # as found; fr30_inv is inlined into k_bary_partial


def test_bary_kernels_use_no_scratch_and_fit_beside_accumulation():
    meta = kernel_meta("bary_kernels.hip")
    found = {}
    for name, m in meta.items():
        for short in VGPRS:
            if short in name:
                found[short] = m
    assert sorted(found) == sorted(VGPRS), sorted(meta)
    for short, m in found.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (short, m)
        assert m["vgpr_count"] <= 160, (short, m)
        assert m["vgpr_count"] == VGPRS[short], (short, m)
    assert found["k_bary_partial"]["group_segment_fixed_size"] <= 40 * 1024  # four workgroups per CU
