"""The barycentric-evaluation kernels (bary_kernels.hip) use no scratch and spill no registers, and stay within the 160 VGPRs
that leave room beside the accumulation kernel; the counts found are pinned.  Checked in the
compiler's metadata for gfx950.  CPU only (hipcc cross-compiles); the assembly is cached under csrc/build/ keyed by the hash
of the sources."""
import hashlib
import os
import re
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kzg_poly_commit_exploration_amd", "csrc")
FLAGS = ["-DKZG_LAZY_FP", "-DKZG_FIPS_SQR", "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S"]
SOURCES = ("bary_kernels.hip", "fr30.hip.h", "engine.h")
VGPRS = {"k_bary_partial": 132, "k_bary_finish": 44}  # as found; fr30_inv is inlined into k_bary_partial


def kernel_meta():
    h = hashlib.sha256()
    for f in SOURCES:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    os.makedirs(os.path.join(CSRC, "build"), exist_ok=True)
    out = os.path.join(CSRC, "build", "bary_kernels_%s.s" % h.hexdigest()[:16])
    if not os.path.exists(out):
        subprocess.run(["hipcc"] + FLAGS + [os.path.join(CSRC, "bary_kernels.hip"), "-o", out], check=True,
                       stderr=subprocess.DEVNULL)
    asm = open(out).read()
    meta = {}
    for block in asm[asm.index("amdhsa.kernels:"):].split("\n  - .")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
                      for key in ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "group_segment_fixed_size")}
    return meta


def test_bary_kernels_use_no_scratch_and_fit_beside_accumulation():
    meta = kernel_meta()
    found = {}
    for name, m in meta.items():
        for short in VGPRS:
            if short in name:
                found[short] = m
    assert sorted(found) == sorted(VGPRS), sorted(meta)
    for short, m in found.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (short, m)
        assert m["vgpr_count"] <= 160, (short, m)
        assert m["vgpr_count"] == VGPRS[short], (short, m)
    assert found["k_bary_partial"]["group_segment_fixed_size"] <= 40 * 1024  # four workgroups per CU
