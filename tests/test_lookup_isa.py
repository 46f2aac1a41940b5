"""The kernels of the log-derivative sums and of the multiplicities (lookup_kernels.hip: k_lu_tile with its twins
k_lu_tile_lookup and k_lu_tile_inv, k_lu_carry, k_lu_finish, k_lu_build, k_lu_probe, k_lu_counts) are the unit's only kernels,
use no scratch memory, spill no register and keep their pinned VGPR counts: checked in the compiler's resource metadata for
gfx950.  The unit is plain HIP C++, without inline assembly.  CPU only (hipcc cross-compiles); the assembly comes from
tests/isa_cache.py.

The goal for every kernel is <= 160 VGPRs (resident beside another slot's accumulation kernel: 512 - 2 x 176).  With a run of 2
rows per lane -- the grand product's run of 4 took 226 -- every kernel meets it: there is no exception to document."""
import os
import re

from isa_cache import CSRC, kernel_meta, requires_hipcc

UNIT = "lookup_kernels.hip"
# as found ("E": the end of the mangled name)
VGPRS = {"k_lu_tileE": 132, "k_lu_tile_lookupE": 132, "k_lu_tile_invE": 99, "k_lu_carryE": 126, "k_lu_finishE": 45,
         "k_lu_buildE": 26, "k_lu_probeE": 26, "k_lu_countsE": 32}
EXCEPTION = set()  # above the goal of 160, below the 256 of two waves per SIMD: none
PLANE = 256 * 9 * 4  # one digit plane of the scans


@requires_hipcc
def test_lookup_kernels_are_listed_and_use_no_scratch():
    meta = kernel_meta(UNIT)
    assert len(meta) == len(VGPRS), sorted(meta)
    by = {}
    for want, vgprs in VGPRS.items():
        found = [k for k in meta if want in k]
        assert len(found) == 1, (want, sorted(meta))
        m = by[want] = meta[found[0]]
        print(found[0], m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
        assert m["vgpr_count"] == vgprs, m
        assert m["vgpr_count"] <= (256 if want in EXCEPTION else 160), m
    for tile in ("k_lu_tileE", "k_lu_tile_lookupE", "k_lu_tile_invE"):
        # two product scans, double-buffered (the additive scan reuses two of the planes), and the word that takes the least row
        assert 4 * PLANE <= by[tile]["group_segment_fixed_size"] <= 4 * PLANE + 64, by[tile]
    # the carry kernel: the same four planes, 1 / D_total, the image of one and the row word
    assert 4 * PLANE <= by["k_lu_carryE"]["group_segment_fixed_size"] <= 4 * PLANE + 128, by["k_lu_carryE"]
    for plain in ("k_lu_finishE", "k_lu_buildE", "k_lu_probeE", "k_lu_countsE"):
        assert by[plain]["group_segment_fixed_size"] == 0, plain


def test_unit_has_no_inline_assembly():
    text = open(os.path.join(CSRC, UNIT)).read()
    assert not re.search(r"\basm\b|__asm", text)
