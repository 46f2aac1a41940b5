"""Every kernel of the MSM sort of a commitment has to fit on a CU BESIDE two workgroups of the accumulation kernel: the
accumulation grid is exactly one resident round, two workgroups per CU, so a kernel that does not fit beside them has to wait
for a CU that one of the two has left (msm_sort.hip, at kRecodeBlock; DESIGN.md sections 4.3 and 5.0s).  This test
reads the registers, LDS and scratch of the sort kernels from the compiler's resource remarks for gfx950 and holds them to what
two accumulation workgroups leave free.  The accumulation kernel's own figures come from its sources: the register clobber in
msm_accum.hip and the LDS reservation in api.hip.  CPU only (hipcc cross-compiles); the remarks come from
tests/isa_cache.py."""
import os
import re

import pytest

from isa_cache import CSRC, remarks_text, requires_hipcc

VGPRS_PER_SIMD_LANE = 512
LDS_PER_CU = 160 * 1024
VGPR_GRANULE = 8
FRONT_KERNELS = ("k_sort_count", "k_sort_spread", "k_sort_spread_staged", "k_fine_count", "k_fine_binscan", "k_fine_scatter")

pytestmark = requires_hipcc


def read(name):
    return open(os.path.join(CSRC, name)).read()


@pytest.fixture(scope="module")
def usage():
    """kernel name -> list of (mangled name, VGPRs and AGPRs (one register file on gfx950), scratch bytes per lane, LDS bytes per
    workgroup), one per instantiation"""
    kernels = {}
    for block in remarks_text("msm_sort.hip", "-Rpass-analysis=kernel-resource-usage").split("Function Name: ")[1:]:
        mangled = block.split()[0]
        m = re.match(r"_ZN3kzg\d+(k_[a-z_]+)", mangled)
        if not m:
            continue
        field = lambda label: int(re.search(re.escape(label) + r":\s+(\d+)", block).group(1))
        kernels.setdefault(m.group(1), []).append(
            (mangled, field("VGPRs") + field("AGPRs"), field("ScratchSize [bytes/lane]"), field("LDS Size [bytes/block]")))
    return kernels


def block_sizes():
    """kernel name -> lanes per workgroup, from the __launch_bounds__ of msm_sort.hip and the constants they name"""
    src = read("msm_sort.hip")
    consts = {k: int(v) for k, v in re.findall(r"constexpr int (k\w+) = (\d+);", src)}
    return {kernel: consts[bound] for bound, kernel in re.findall(r"__launch_bounds__\((k\w+)\)\s+(k_\w+)\(", src)}


def accumulation_footprint():
    """(VGPRs, LDS bytes) of one accumulation workgroup's waves: the clobber that reserves v0..vN, the context's reservation"""
    vgprs = int(re.search(r'asm volatile\(""\s*:::\s*"v(\d+)"\)', read("msm_accum.hip")).group(1)) + 1
    lds = int(re.search(r"accum_lds_bytes = (\d+)u \* 1024u;", read("api.hip")).group(1)) * 1024
    accum_block = int(re.search(r"#define KZG_ACCUM_BLOCK (\d+)", read("msm_accum.hip")).group(1))
    assert accum_block == 256, "one wave per SIMD and workgroup is what the budget below counts"
    return vgprs, lds


def test_sources_name_what_the_budget_is_taken_from():
    vgprs, lds = accumulation_footprint()
    assert 128 < vgprs <= 256 and vgprs % VGPR_GRANULE == 0  # two workgroups per CU, not three, not one
    assert 0 < lds < LDS_PER_CU // 2
    sizes = block_sizes()
    assert set(FRONT_KERNELS) <= set(sizes), sizes


@pytest.mark.parametrize("kernel", FRONT_KERNELS)
def test_front_kernel_fits_beside_two_accumulation_workgroups(usage, kernel):
    accum_vgprs, accum_lds = accumulation_footprint()
    free_vgprs = VGPRS_PER_SIMD_LANE - 2 * accum_vgprs
    free_lds = LDS_PER_CU - 2 * accum_lds
    lanes = block_sizes()[kernel]
    waves_per_simd = -(-lanes // 256)
    assert usage.get(kernel), "no resource remark for %s" % kernel
    for mangled, vgprs, scratch, lds in usage[kernel]:
        allocated = -(-vgprs // VGPR_GRANULE) * VGPR_GRANULE
        print("%s: %d lanes, %d VGPRs (%d allocated) x %d = %d of %d, LDS %d of %d, scratch %d"
              % (mangled, lanes, vgprs, allocated, waves_per_simd, waves_per_simd * allocated, free_vgprs, lds, free_lds, scratch))
        assert waves_per_simd * allocated <= free_vgprs, mangled
        assert lds <= free_lds, mangled
        assert scratch == 0, mangled


def test_every_width_of_the_recoding_kernels_is_compiled(usage):
    # the run-time loop (0) and the widths choose_msm_config picks at 2^17 ... 2^22 terms
    for kernel in ("k_sort_count", "k_sort_spread", "k_sort_spread_staged"):
        widths = sorted(int(re.search(kernel + r"ILj(\d+)E", m).group(1)) for m, _, _, _ in usage[kernel])
        assert widths == [0, 15, 16, 17, 19], (kernel, widths)
    assert len(usage["k_fine_count"]) == 2 and len(usage["k_fine_scatter"]) == 2  # packed and two-word pairs
