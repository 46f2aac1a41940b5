"""The multiproof kernels (poly_kernels.hip: k_points_*) use no scratch memory: checked in the compiler's metadata for gfx950.
CPU only (hipcc cross-compiles); the assembly comes from tests/isa_cache.py."""
from isa_cache import kernel_meta, requires_hipcc


@requires_hipcc
def test_points_kernels_use_no_scratch():
    meta = kernel_meta("poly_kernels.hip")
    points = {k: v for k, v in meta.items() if "k_points_" in k}
    assert len(points) == 3, sorted(meta)
    for name, m in points.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
