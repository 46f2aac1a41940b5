"""The kernels of a circuit's lookup argument (lookup_circuit_kernels.hip: k_lk_fold, k_lk_constraints) are the unit's only kernels,
use no scratch memory and no LDS, spill no register and keep their pinned VGPR counts: checked in the compiler's resource metadata
for gfx950.  The unit is plain HIP C++, without inline assembly.  CPU only (hipcc cross-compiles); the assembly comes from
tests/isa_cache.py.

The rule is <= 160 VGPRs (resident beside another slot's accumulation kernel: 512 - 2 x 176).  Both kernels walk their columns with
loops that are not unrolled and hold one folded sum at a time beside the product's own registers."""
import os
import re

from isa_cache import CSRC, kernel_meta, requires_hipcc

UNIT = "lookup_circuit_kernels.hip"
VGPRS = {"k_lk_foldE": 58, "k_lk_constraintsE": 77}  # as found ("E": the end of the mangled name)


@requires_hipcc
def test_lookup_circuit_kernels_are_listed_and_use_no_scratch():
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


def test_the_column_loop_is_not_unrolled_and_offsets_are_64_bit():
    text = open(os.path.join(CSRC, UNIT)).read()
    assert re.search(r"#pragma unroll 1\n\s+for \(uint32_t j = 0; j < c; j\+\+\)", text)
    body = text[text.index("__global__"):]
    assert "8 * i" not in body and body.count("8 * (size_t)i") >= 8  # every row offset is formed in 64 bits
