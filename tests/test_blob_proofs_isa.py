"""The batched quotient kernel of blob proofs (blobproof_kernels.hip: k_blobproof_quotients) is the unit's only kernel, uses no
scratch memory, spills no register and keeps its pinned VGPR count: checked in the compiler's resource metadata for gfx950.  The
unit is plain HIP C++, without inline assembly.  CPU only (hipcc cross-compiles); the assembly comes from tests/isa_cache.py."""
import os
import re

from isa_cache import CSRC, kernel_meta, requires_hipcc

UNIT = "blobproof_kernels.hip"
VGPRS = {"k_blobproof_quotients": 66}  # as found


@requires_hipcc
def test_blobproof_kernels_are_listed_and_use_no_scratch():
    meta = kernel_meta(UNIT)
    assert len(meta) == len(VGPRS), sorted(meta)
    for want, vgprs in VGPRS.items():
        found = [k for k in meta if want in k]
        assert len(found) == 1, (want, sorted(meta))
        m = meta[found[0]]
        print(found[0], m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
        assert m["vgpr_count"] == vgprs, m
        assert 256 * 9 * 4 <= m["group_segment_fixed_size"] <= 16384, m  # the scan's exchange, statically sized
    for name in meta:  # the ISA tests of the scans pick their kernels by these substrings
        assert "k_points_" not in name and "k_sets_" not in name


def test_unit_has_no_inline_assembly():
    text = open(os.path.join(CSRC, UNIT)).read()
    assert not re.search(r"\basm\b|__asm", text)
