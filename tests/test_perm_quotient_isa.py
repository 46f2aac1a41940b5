"""The kernels of the permutation quotient (quotient_kernels.hip: k_pq_constraints, k_pq_pad_twist) are the unit's only kernels,
use no scratch memory and no LDS, spill no register and keep their pinned VGPR counts: checked in the compiler's resource metadata
for gfx950.  The unit is plain HIP C++, without inline assembly.  CPU only (hipcc cross-compiles); the assembly comes from
tests/isa_cache.py.

The goal was <= 160 VGPRs (resident beside another slot's accumulation kernel: 512 - 2 x 176).  Both kernels meet it: the columns
of k_pq_constraints are walked by a loop that is not unrolled, so its register state does not grow with t."""
import os
import re

from isa_cache import CSRC, kernel_meta, requires_hipcc

UNIT = "quotient_kernels.hip"
VGPRS = {"k_pq_constraintsE": 103, "k_pq_pad_twistE": 56}  # as found ("E": the end of the mangled name)


@requires_hipcc
def test_quotient_kernels_are_listed_and_use_no_scratch():
    meta = kernel_meta(UNIT)
    assert len(meta) == len(VGPRS), sorted(meta)
    for want, vgprs in VGPRS.items():
        found = [k for k in meta if want in k]
        assert len(found) == 1, (want, sorted(meta))
        m = meta[found[0]]
        print(found[0], m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
        assert m["group_segment_fixed_size"] == 0, m
        assert m["vgpr_count"] == vgprs and m["vgpr_count"] <= 160, m


def test_unit_has_no_inline_assembly():
    text = open(os.path.join(CSRC, UNIT)).read()
    assert not re.search(r"\basm\b|__asm", text)


def test_the_tile_the_gpu_tests_read_is_the_units():
    text = open(os.path.join(CSRC, "engine.h")).read()
    assert re.search(r"constexpr uint32_t kPqTile = 256;", text)
