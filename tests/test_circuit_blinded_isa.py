"""The kernels of the blinding (blind_kernels.hip: k_blind_patch, k_blind_tail) are the unit's only kernels, use no scratch memory,
spill no register and keep their pinned VGPR counts: checked in the compiler's resource metadata for gfx950.  CPU only (hipcc
cross-compiles); the assembly is cached under csrc/build/ keyed by the hash of the sources.

The rule is <= 160 VGPRs (resident beside another slot's accumulation kernel: 512 - 2 x 176)."""
import hashlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kzg_poly_commit_exploration_amd", "csrc")
FLAGS = ["-DKZG_LAZY_FP", "-DKZG_FIPS_SQR", "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S"]
UNIT = "blind_kernels.hip"
VGPRS = {"k_blind_patchE": 51, "k_blind_tailE": 60}  # as found ("E": the end of the mangled name)


def kernel_meta():
    h = hashlib.sha256()
    for f in (UNIT, "combine_lanes.hip.h", "fr30.hip.h", "engine.h"):
        h.update(open(os.path.join(CSRC, f), "rb").read())
    os.makedirs(os.path.join(CSRC, "build"), exist_ok=True)
    out = os.path.join(CSRC, "build", "blind_kernels_%s.s" % h.hexdigest()[:16])
    if not os.path.exists(out):
        subprocess.run(["hipcc"] + FLAGS + [os.path.join(CSRC, UNIT), "-o", out], check=True, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    meta = {}
    for block in asm[asm.index("amdhsa.kernels:"):].split("\n  - .")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
                      for key in ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    return meta


@pytest.mark.skipif(subprocess.run(["which", "hipcc"], capture_output=True).returncode != 0, reason="no hipcc")
def test_blind_kernels_are_listed_and_use_no_scratch():
    meta = kernel_meta()
    assert len(meta) == len(VGPRS), sorted(meta)
    for want, vgprs in VGPRS.items():
        found = [k for k in meta if want in k]
        assert len(found) == 1, (want, sorted(meta))
        m = meta[found[0]]
        print(found[0], m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
        assert m["vgpr_count"] == vgprs and m["vgpr_count"] <= 160, m


def test_unit_has_no_inline_assembly():
    text = open(os.path.join(CSRC, UNIT)).read()
    assert not re.search(r"\basm\b|__asm", text)
