"""The batched NTT pass kernel (ntt_batch_kernels.hip: k_nttb_pass) is the unit's only kernel, stays within the 128 VGPRs of
k_ntt_pass's limit (two 256-thread workgroups per CU), uses no scratch memory and spills nothing: read from the compiler's
metadata for gfx950.  CPU only (hipcc cross-compiles); the assembly comes from tests/isa_cache.py."""
import os
import re

from isa_cache import CSRC, kernel_meta, requires_hipcc


@requires_hipcc
def test_one_kernel_within_the_pass_kernels_limits():
    meta = kernel_meta("ntt_batch_kernels.hip")
    assert len(meta) == 1, sorted(meta)
    (name, m), = meta.items()
    assert "k_nttb_pass" in name and "k_ntt_pass" not in name, name  # (tests/test_ntt_isa.py counts the latter)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
    assert m["vgpr_count"] <= 128, (name, m)


def test_the_unit_is_built_into_the_library():
    srcs = re.search(r"^SRCS\s*=(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert "ntt_batch_kernels.hip" in srcs
