"""The encoders' kernels (blob_kernels.hip) use no scratch and spill no registers; the VGPR counts found
are pinned.  They run behind a batch of proofs or a transform, not beside an accumulation, so the 160-VGPR rule of DESIGN.md
section 4.4 is not asked of them (they meet it all the same).  Checked in the compiler's metadata for gfx950.  CPU only (hipcc
cross-compiles); the assembly comes from tests/isa_cache.py.  The tree-wide check for scalar
stores is test_wire_bytes_isa.py's: it walks the new files with the rest."""
import os
import re

from isa_cache import CSRC, kernel_meta

UNIT = "blob_kernels.hip"
VGPRS = {"k_enc_g1": 76, "k_enc_fr": 41, "k_poly_trim": 47}  # as found


def test_blob_kernels_use_no_scratch_and_spill_nothing():
    meta = kernel_meta(UNIT)
    assert len(meta) == len(VGPRS), sorted(meta)  # every kernel of the unit is listed here
    found = {short: m for name, m in meta.items() for short in VGPRS if short in name}
    assert sorted(found) == sorted(VGPRS), sorted(meta)
    for short, m in found.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (short, m)
        assert m["vgpr_count"] == VGPRS[short], (short, m)


def test_the_unit_has_no_inline_assembly():
    for f in (UNIT, "wire_enc30.hip.h"):
        text = open(os.path.join(CSRC, f)).read()
        assert not re.search(r"\basm\b|__asm", text), f
