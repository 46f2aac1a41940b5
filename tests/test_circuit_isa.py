"""The kernel of the circuit quotient (circuit_kernels.hip: k_ck_constraints) is the unit's only kernel, uses no scratch memory and
no LDS, spills no register and keeps its pinned VGPR count: checked in the compiler's resource metadata for gfx950.  The unit is
plain HIP C++, without inline assembly.  CPU only (hipcc cross-compiles); the assembly comes from tests/isa_cache.py.

The rule is <= 160 VGPRs (resident beside another slot's accumulation kernel: 512 - 2 x 176).  The fused kernel meets it: the
columns are walked by a loop that is not unrolled, so beside k_pq_constraints' state (103) it holds only the gate's sum, f_0 and
the scaling constant."""
import os
import re

from isa_cache import CSRC, kernel_meta, requires_hipcc

UNIT = "circuit_kernels.hip"
VGPRS = {"k_ck_constraintsE": 128}  # as found ("E": the end of the mangled name)


@requires_hipcc
def test_circuit_kernels_are_listed_and_use_no_scratch():
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


def test_the_column_loop_is_not_unrolled():
    text = open(os.path.join(CSRC, UNIT)).read()
    body = text[text.index("k_ck_constraints(CkArgs in"):]
    assert re.search(r"#pragma unroll 1\n\s+for \(uint32_t j = 0; j < in\.t; j\+\+\)", body)
