"""The two kernels of the evaluation-form quotient (lagrange_kernels.hip: k_lagrange_partial, k_lagrange_finish) are the unit's
only kernels, use no scratch memory, spill no register and keep their pinned VGPR counts: checked in the compiler's resource
metadata for gfx950.  The unit is plain HIP C++, without inline assembly.  CPU only (hipcc cross-compiles); the assembly
comes from tests/isa_cache.py."""
import os
import re

from isa_cache import CSRC, kernel_meta, requires_hipcc

UNIT = "lagrange_kernels.hip"
VGPRS = {"k_lagrange_partial": 142, "k_lagrange_finish": 66}  # as found; the goal for the partial kernel was <= 160
PLANE = 256 * 9 * 4  # one digit plane of the tile's scans


@requires_hipcc
def test_lagrange_kernels_are_listed_and_use_no_scratch():
    meta = kernel_meta(UNIT)
    assert len(meta) == len(VGPRS), sorted(meta)
    for want, vgprs in VGPRS.items():
        found = [k for k in meta if want in k]
        assert len(found) == 1, (want, sorted(meta))
        m = meta[found[0]]
        print(found[0], m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
        assert m["vgpr_count"] == vgprs, m
    partial = meta[[k for k in meta if "k_lagrange_partial" in k][0]]
    assert partial["vgpr_count"] <= 160  # resident beside the accumulation kernel of another slot: 512 - 2 x 176
    assert 4 * PLANE <= partial["group_segment_fixed_size"] <= 4 * PLANE + 256, partial  # two scans, double-buffered


def test_unit_has_no_inline_assembly():
    text = open(os.path.join(CSRC, UNIT)).read()
    assert not re.search(r"\basm\b|__asm", text)
