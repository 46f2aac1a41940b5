"""The kernels of the openings at several point sets (combine_kernels.hip: k_sets_combine; poly_kernels.hip: k_sets_chunks,
k_sets_blocks, k_sets_apply) use no scratch memory and spill no register: checked in the compiler's metadata for gfx950.
CPU only (hipcc cross-compiles); the assembly is cached under csrc/build/ keyed by the hash of the sources."""
import hashlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kzg_poly_commit_exploration_amd", "csrc")
FLAGS = ["-DKZG_LAZY_FP", "-DKZG_FIPS_SQR", "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S"]
UNITS = {"combine_kernels.hip": ["k_sets_combine"], "poly_kernels.hip": ["k_sets_chunks", "k_sets_blocks", "k_sets_apply"]}


def kernel_meta(unit):
    h = hashlib.sha256()
    for f in (unit, "fr30.hip.h", "fr30_host.hpp", "engine.h"):
        h.update(open(os.path.join(CSRC, f), "rb").read())
    os.makedirs(os.path.join(CSRC, "build"), exist_ok=True)
    out = os.path.join(CSRC, "build", "%s_sets_%s.s" % (unit.split(".")[0], h.hexdigest()[:16]))
    if not os.path.exists(out):
        subprocess.run(["hipcc"] + FLAGS + [os.path.join(CSRC, unit), "-o", out], check=True, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    meta = {}
    for block in asm[asm.index("amdhsa.kernels:"):].split("\n  - .")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
                      for key in ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count")}
    return meta


@pytest.mark.skipif(subprocess.run(["which", "hipcc"], capture_output=True).returncode != 0, reason="no hipcc")
@pytest.mark.parametrize("unit", sorted(UNITS))
def test_sets_kernels_use_no_scratch(unit):
    meta = kernel_meta(unit)
    sets = {k: v for k, v in meta.items() if "k_sets_" in k}
    for want in UNITS[unit]:
        assert sum(want in k for k in sets) == 1, (want, sorted(meta))
    assert len(sets) == len(UNITS[unit]), sorted(sets)
    for name, m in sets.items():
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
