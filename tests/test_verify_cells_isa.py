"""The batch-verification kernels (verify_kernels.hip) use no scratch and spill no registers; the Fr kernels also stay within 160
VGPRs.  The ladder kernels are latency-bound like the G1 DFT stages and take the registers they need.  Checked in the
compiler's metadata for gfx950.  CPU only (hipcc
cross-compiles); the assembly is cached under csrc/build/ keyed by the hash of the sources."""
import hashlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kzg_poly_commit_exploration_amd", "csrc")
FLAGS = ["-DKZG_LAZY_FP", "-DKZG_FIPS_SQR", "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S"]
SOURCES = ("verify_kernels.hip", "fr30.hip.h", "engine.h", "g1_30.hip.h", "field30.hip.h")


def kernel_meta():
    h = hashlib.sha256()
    for f in SOURCES:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    os.makedirs(os.path.join(CSRC, "build"), exist_ok=True)
    out = os.path.join(CSRC, "build", "recover_kernels_%s.s" % h.hexdigest()[:16])
    if not os.path.exists(out):
        subprocess.run(["hipcc"] + FLAGS + [os.path.join(CSRC, "verify_kernels.hip"), "-o", out], check=True,
                       stderr=subprocess.DEVNULL)
    asm = open(out).read()
    meta = {}
    for block in asm[asm.index("amdhsa.kernels:"):].split("\n  - .")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
                      for key in ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count")}
    return meta


@pytest.mark.skipif(subprocess.run(["which", "hipcc"], capture_output=True).returncode != 0, reason="no hipcc")
def test_verify_kernels_use_no_scratch():
    meta = kernel_meta()
    rec = {k: v for k, v in meta.items() if "k_vc_" in k}
    assert len(rec) == 5, sorted(meta)
    for name, m in rec.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        if "_fr_" in name:
            assert m["vgpr_count"] <= 160, (name, m)
