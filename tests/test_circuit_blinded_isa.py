"""The kernels of the blinding (blind_kernels.hip: k_blind_patch, k_blind_tail) are the unit's only kernels, use no scratch memory,
spill no register and keep their pinned VGPR counts: checked in the compiler's resource metadata for gfx950.  CPU only (hipcc
cross-compiles); the assembly comes from tests/isa_cache.py.

The rule is <= 160 VGPRs (resident beside another slot's accumulation kernel: 512 - 2 x 176)."""
import os
import re

from isa_cache import CSRC, kernel_meta, requires_hipcc

UNIT = "blind_kernels.hip"
VGPRS = {"k_blind_patchE": 51, "k_blind_tailE": 60}  # as found ("E": the end of the mangled name)


@requires_hipcc
def test_blind_kernels_are_listed_and_use_no_scratch():
    meta = kernel_meta(UNIT)
    assert len(meta) == len(VGPRS), sorted(meta)
    for want, vgprs in VGPRS.items():
        found = [k for k in meta if want in k]
        assert len(found) == 1, (want, sorted(meta))
        m = meta[found[0]]
        print(found[0], m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
        assert m["vgpr_count"] == vgprs and m["vgpr_count"] <= 160, m


def test_unit_has_no_inline_assembly():
    text = open(os.path.join(CSRC, UNIT)).read()
    assert not re.search(r"\basm\b|__asm", text)
