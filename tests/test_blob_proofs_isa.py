"""The batched quotient kernel of blob proofs (blobproof_kernels.hip: k_blobproof_quotients) is the unit's only kernel, uses no
scratch memory, spills no register and keeps its pinned VGPR count: checked in the compiler's resource metadata for gfx950.  The
unit is plain HIP C++, without inline assembly.  CPU only (hipcc cross-compiles); the assembly is cached under csrc/build/ keyed
by the hash of the sources."""
import hashlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kzg_poly_commit_exploration_amd", "csrc")
FLAGS = ["-DKZG_LAZY_FP", "-DKZG_FIPS_SQR", "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S"]
UNIT = "blobproof_kernels.hip"
VGPRS = {"k_blobproof_quotients": 66}  # as found


def kernel_meta():
    h = hashlib.sha256()
    for f in (UNIT, "fr30.hip.h", "engine.h"):
        h.update(open(os.path.join(CSRC, f), "rb").read())
    os.makedirs(os.path.join(CSRC, "build"), exist_ok=True)
    out = os.path.join(CSRC, "build", "blobproof_kernels_%s.s" % h.hexdigest()[:16])
    if not os.path.exists(out):
        subprocess.run(["hipcc"] + FLAGS + [os.path.join(CSRC, UNIT), "-o", out], check=True, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    meta = {}
    for block in asm[asm.index("amdhsa.kernels:"):].split("\n  - .")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
                      for key in ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                  "group_segment_fixed_size")}
    return meta


@pytest.mark.skipif(subprocess.run(["which", "hipcc"], capture_output=True).returncode != 0, reason="no hipcc")
def test_blobproof_kernels_are_listed_and_use_no_scratch():
    meta = kernel_meta()
    assert len(meta) == len(VGPRS), sorted(meta)
    for want, vgprs in VGPRS.items():
        found = [k for k in meta if want in k]
        assert len(found) == 1, (want, sorted(meta))
        m = meta[found[0]]
        print(found[0], m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
        assert m["vgpr_count"] == vgprs, m
        assert 256 * 9 * 4 <= m["group_segment_fixed_size"] <= 16384, m  # the scan's exchange, statically sized
    for name in meta:  # the ISA tests of the scans pick their kernels by these substrings
        assert "k_points_" not in name and "k_sets_" not in name


def test_unit_has_no_inline_assembly():
    text = open(os.path.join(CSRC, UNIT)).read()
    assert not re.search(r"\basm\b|__asm", text)
