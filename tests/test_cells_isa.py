"""The cell kernels (cell_kernels.hip) use no scratch and at most 160 VGPRs, what fits beside the accumulation kernel's two
waves per SIMD: checked in the compiler's metadata for gfx950.  CPU only (hipcc cross-compiles); the assembly comes from
tests/isa_cache.py."""
from isa_cache import kernel_meta, requires_hipcc


@requires_hipcc
def test_cell_kernels_fit_beside_the_accumulation():
    meta = kernel_meta("cell_kernels.hip")
    cells = {k: v for k, v in meta.items() if "k_cells_" in k}
    assert len(cells) == 3, sorted(meta)
    for name, m in cells.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 160, (name, m)
