"""The encoders' kernels (blob_kernels.hip) use no scratch and spill no registers; the VGPR counts found
are pinned.  They run behind a batch of proofs or a transform, not beside an accumulation, so the 160-VGPR rule of DESIGN.md
section 4.4 is not asked of them (they meet it all the same).  Checked in the compiler's metadata for gfx950.  CPU only (hipcc
cross-compiles); the assembly is cached under csrc/build/ keyed by the hash of the sources.  The tree-wide check for scalar
stores is test_wire_bytes_isa.py's: it walks the new files with the rest."""
import hashlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kzg_poly_commit_exploration_amd", "csrc")
FLAGS = ["-DKZG_LAZY_FP", "-DKZG_FIPS_SQR", "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S"]
HEADERS = tuple(sorted(f for f in os.listdir(CSRC) if f.endswith((".h", ".hpp", ".inc"))))  # whatever a unit may include
UNIT = "blob_kernels.hip"
VGPRS = {"k_enc_g1": 76, "k_enc_fr": 41, "k_poly_trim": 47}  # as found


def kernel_meta(unit):
    h = hashlib.sha256()
    for f in (unit,) + HEADERS:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    os.makedirs(os.path.join(CSRC, "build"), exist_ok=True)
    out = os.path.join(CSRC, "build", "%s_%s.s" % (unit.split(".")[0], h.hexdigest()[:16]))
    if not os.path.exists(out):
        subprocess.run(["hipcc"] + FLAGS + [os.path.join(CSRC, unit), "-o", out], check=True, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    meta = {}
    for block in asm[asm.index("amdhsa.kernels:"):].split("\n  - .")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
                      for key in ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    return meta


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
