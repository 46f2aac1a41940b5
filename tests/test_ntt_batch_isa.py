"""The batched NTT pass kernel (ntt_batch_kernels.hip: k_nttb_pass) is the unit's only kernel, stays within the 128 VGPRs of
k_ntt_pass's limit (two 256-thread workgroups per CU), uses no scratch memory and spills nothing: read from the compiler's
metadata for gfx950.  CPU only (hipcc cross-compiles); the assembly is cached under csrc/build/ keyed by the sources."""
import hashlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kzg_poly_commit_exploration_amd", "csrc")
FLAGS = ["-DKZG_LAZY_FP", "-DKZG_FIPS_SQR", "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S"]


def kernel_meta():
    h = hashlib.sha256()
    for f in ("ntt_batch_kernels.hip", "fr30.hip.h", "engine.h"):
        h.update(open(os.path.join(CSRC, f), "rb").read())
    os.makedirs(os.path.join(CSRC, "build"), exist_ok=True)
    out = os.path.join(CSRC, "build", "ntt_batch_kernels_%s.s" % h.hexdigest()[:16])
    if not os.path.exists(out):
        subprocess.run(["hipcc"] + FLAGS + [os.path.join(CSRC, "ntt_batch_kernels.hip"), "-o", out], check=True,
                       stderr=subprocess.DEVNULL)
    asm = open(out).read()
    meta = {}
    for block in asm[asm.index("amdhsa.kernels:"):].split("\n  - .")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
                      for key in ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    return meta


@pytest.mark.skipif(subprocess.run(["which", "hipcc"], capture_output=True).returncode != 0, reason="no hipcc")
def test_one_kernel_within_the_pass_kernels_limits():
    meta = kernel_meta()
    assert len(meta) == 1, sorted(meta)
    (name, m), = meta.items()
    assert "k_nttb_pass" in name and "k_ntt_pass" not in name, name  # (tests/test_ntt_isa.py counts the latter)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
    assert m["vgpr_count"] <= 128, (name, m)


def test_the_unit_is_built_into_the_library():
    srcs = re.search(r"^SRCS\s*=(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert "ntt_batch_kernels.hip" in srcs
