"""The FK20 kernels (fk20_kernels.hip) use no scratch and spill no registers: checked in the compiler's metadata for gfx950.
They carry no 160-VGPR cap: the latency-bound DFT stages and the comb builder run on their own, not beside the accumulation
kernel (DESIGN.md section 4.8 lists the counts).  CPU only (hipcc cross-compiles); the assembly comes from
tests/isa_cache.py."""
import re

from isa_cache import kernel_meta, requires_hipcc


@requires_hipcc
def test_fk20_kernels_use_no_scratch():
    meta = kernel_meta("fk20_kernels.hip")
    fk = {k: v for k, v in meta.items() if re.search(r"k_(g1_|fk20_|fr_stage)", k)}
    assert len(fk) == 10, sorted(meta)
    for name, m in fk.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 512, (name, m)
