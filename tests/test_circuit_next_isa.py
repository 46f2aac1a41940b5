"""The kernel of a next-row circuit's custom gates (custom_next_kernels.hip: k_cgn_gate) stays within the
rule for light kernels of <= 160 VGPRs (resident beside another slot's accumulation kernel: 512 - 2 x 176), uses no scratch memory
and spills no register: checked in the compiler's resource metadata for gfx950, compiled with the Makefile's flags through
tests/isa_cache.py.  CPU only (hipcc cross-compiles).  Only these resource figures are asserted."""
from isa_cache import kernel_meta, requires_hipcc

UNIT = "custom_next_kernels.hip"
KERNEL = "k_cgn_gateE"  # ("E": the end of the mangled name)


@requires_hipcc
def test_next_row_gate_kernel_stays_light_and_uses_no_scratch():
    meta = kernel_meta(UNIT)
    found = [k for k in meta if KERNEL in k]
    assert len(found) == 1, sorted(meta)
    m = meta[found[0]]
    print(found[0], m)
    assert m["vgpr_count"] <= 160, m
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
