"""The kernels of the linearisation (linearise_kernels.hip: k_lin_combine, k_lin_finish) are the unit's only kernels, use no scratch
memory, spill no register and keep their pinned VGPR counts: checked in the compiler's resource metadata for gfx950.  The unit is
plain HIP C++, without inline assembly, and the column loop is not unrolled.  CPU only (hipcc cross-compiles); the assembly comes from
tests/isa_cache.py.

The rule is <= 160 VGPRs (resident beside another slot's accumulation kernel: 512 - 2 x 176).  k_lin_combine meets it because a lane
takes its eight indices in two halves of four: four accumulators and eight loads in flight (with the whole run at once the compiler
asked for 226)."""
import os
import re

from isa_cache import CSRC, kernel_meta, requires_hipcc

UNIT = "linearise_kernels.hip"
VGPRS = {"k_lin_combineE": 148, "k_lin_finishE": 56}  # as found ("E": the end of the mangled name)
LDS_BYTES = 9 * 4 * 4  # the workgroup sum: nine digits of four wave totals


@requires_hipcc
def test_linearise_kernels_are_listed_and_use_no_scratch():
    meta = kernel_meta(UNIT)
    assert len(meta) == len(VGPRS), sorted(meta)
    for want, vgprs in VGPRS.items():
        found = [k for k in meta if want in k]
        assert len(found) == 1, (want, sorted(meta))
        m = meta[found[0]]
        print(found[0], m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
        assert m["group_segment_fixed_size"] == LDS_BYTES, m  # no LDS beyond the workgroup sum
        assert m["vgpr_count"] == vgprs and m["vgpr_count"] <= 160, m


def test_unit_has_no_inline_assembly():
    text = open(os.path.join(CSRC, UNIT)).read()
    assert not re.search(r"\basm\b|__asm", text)


def test_the_column_loop_is_not_unrolled():
    text = open(os.path.join(CSRC, UNIT)).read()
    body = text[text.index("k_lin_combine(const LinColumn*"):]
    assert re.search(r"#pragma unroll 1\n\s+for \(uint32_t k = 0; k < ncols; k\+\+\)", body)
