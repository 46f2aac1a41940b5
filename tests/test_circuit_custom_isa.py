"""The kernel of a circuit's custom gates (custom_gate_kernels.hip: k_cg_gate) is the unit's only kernel, uses no scratch memory and
no LDS, spills no register and keeps its pinned VGPR count: checked in the compiler's resource metadata for gfx950.  The unit is
plain HIP C++, without inline assembly.  CPU only (hipcc cross-compiles); the assembly comes from tests/isa_cache.py.

The rule is <= 160 VGPRs (resident beside another slot's accumulation kernel: 512 - 2 x 176).  The kernel walks its terms, wires
and exponents with loops that are not unrolled and holds the running sum, one term and one wire's multiplier form beside the
product's own registers: no array of wires is indexed by a loop variable, which is what would send it to scratch memory."""
import os
import re

from isa_cache import CSRC, kernel_meta, requires_hipcc

UNIT = "custom_gate_kernels.hip"
VGPRS = {"k_cg_gateE": 84}  # as found ("E": the end of the mangled name)


@requires_hipcc
def test_custom_gate_kernel_is_listed_and_uses_no_scratch():
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


def test_the_loops_are_not_unrolled_and_offsets_are_64_bit():
    text = open(os.path.join(CSRC, UNIT)).read()
    body = text[text.index("__global__"):text.index("}  // namespace")]
    for loop in (r"for \(uint32_t s = 0; s < in\.g; s\+\+\)", r"for \(uint32_t j = 0; j < in\.t; j\+\+\)", r"for \(uint32_t k = 0; k < p; k\+\+\)"):
        assert re.search(r"#pragma unroll 1\n\s+" + loop, body), loop
    assert not re.search(r"8 \* i\b", body) and body.count("8 * (size_t)i") >= 3  # every point offset is formed in 64 bits
    assert "8 * (size_t)in.N" in body and "8 * in.stride" in body and "size_t stride;" in text  # and every column step
