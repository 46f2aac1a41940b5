"""The wire decoders' kernels (wire_kernels.hip, and k_uncompress of srs_io.hip which runs the same decoder) use no scratch and
spill no registers; the VGPR counts found are pinned.  They run in front of a verification, not beside an accumulation, so the
160-VGPR rule of DESIGN.md section 4.4 is not asked of them (they meet it all the same).  Checked in the compiler's metadata
for gfx950.  CPU only (hipcc cross-compiles); the assembly is cached under csrc/build/ keyed by the hash of the sources.
Also: no source file of the tree names a scalar store or a scalar-cache write-back."""
import hashlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kzg_poly_commit_exploration_amd", "csrc")
FLAGS = ["-DKZG_LAZY_FP", "-DKZG_FIPS_SQR", "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S"]
HEADERS = tuple(sorted(f for f in os.listdir(CSRC) if f.endswith((".h", ".hpp", ".inc"))))  # whatever a unit may include
VGPRS = {"wire_kernels.hip": {"k_wire_g1": 118, "k_wire_fr": 43}, "srs_io.hip": {"k_uncompress": 118}}  # as found


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


def test_wire_kernels_use_no_scratch_and_spill_nothing():
    for unit, want in VGPRS.items():
        meta = kernel_meta(unit)
        found = {short: m for name, m in meta.items() for short in want if short in name}
        assert sorted(found) == sorted(want), sorted(meta)
        for short, m in found.items():
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (short, m)
            assert m["vgpr_count"] == want[short], (short, m)


def test_no_scalar_stores_in_the_tree():
    """scalar stores to memory, scalar atomics and the scalar cache's write-back are not used anywhere: not in code, not in
    strings, not in comments (documents may speak of them)"""
    words = [a + b for a in ("s_", "s_buffer_", "s_scratch_") for b in ("store", "atomic")] + ["s_dcache_" + "wb", "s_dcache_" + "discard"]
    pat = re.compile(r"\b(" + "|".join(words) + ")", re.IGNORECASE)  # (points_store_sums is a function of poly_kernels.hip)
    hits = []
    source = (".hip", ".h", ".hpp", ".cpp", ".c", ".cc", ".inc", ".py", ".sh", ".cmake", ".s", ".S", ".asm", ".rs")
    for base, dirs, files in os.walk(ROOT):
        dirs[:] = [d for d in dirs if not d.startswith(".") and d not in ("build", "__pycache__", "_ref")]
        for f in files:
            if not (f.endswith(source) or f in ("Makefile", "CMakeLists.txt")):
                continue
            path = os.path.join(base, f)
            try:
                text = open(path, encoding="utf-8", errors="ignore").read()
            except OSError:
                continue
            if pat.search(text):
                hits.append(os.path.relpath(path, ROOT))
    assert not hits, hits
