"""The kernels of the openings at several point sets (combine_kernels.hip: k_sets_combine; poly_kernels.hip: k_sets_chunks,
k_sets_blocks, k_sets_apply) use no scratch memory and spill no register: checked in the compiler's metadata for gfx950.
CPU only (hipcc cross-compiles); the assembly comes from tests/isa_cache.py."""
import pytest

from isa_cache import kernel_meta, requires_hipcc

UNITS = {"combine_kernels.hip": ["k_sets_combine"], "poly_kernels.hip": ["k_sets_chunks", "k_sets_blocks", "k_sets_apply"]}


@requires_hipcc
@pytest.mark.parametrize("unit", sorted(UNITS))
def test_sets_kernels_use_no_scratch(unit):
    meta = kernel_meta(unit)
    sets = {k: v for k, v in meta.items() if "k_sets_" in k}
    for want in UNITS[unit]:
        assert sum(want in k for k in sets) == 1, (want, sorted(meta))
    assert len(sets) == len(UNITS[unit]), sorted(sets)
    for name, m in sets.items():
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
