"""The compiler's output for a kernel unit of csrc/, for the tests that read it (tests/test_*_isa.py, test_front_residency.py,
test_srs_ceremony.py): the flags, the cache key, the cache and the metadata parser, once.  CPU only (hipcc cross-compiles).

The flags are the HIPFLAGS line of csrc/Makefile, read from the file, with --cuda-device-only -S behind it: the tests look at
the code that ships.  The artefact is cached as csrc/build/<unit stem>_<key>.s (.txt for captured remarks); the key is a hash
of the flags, of `hipcc --version`, of the unit and of EVERY header of csrc/ and the public header, so no test keeps a list of
what its unit includes.  A header edit recompiles every unit.  An artefact is written under a temporary name and renamed into
place, so a file under the final name is always a whole one."""
import functools
import hashlib
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kzg_poly_commit_exploration_amd", "csrc")
BUILD = os.path.join(CSRC, "build")

requires_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")


@functools.lru_cache(maxsize=None)
def flags(*extra):
    """csrc/Makefile's HIPFLAGS with its default ARCH, --cuda-device-only -S, then `extra`"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    line = re.search(r"^HIPFLAGS\s*\?=(.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    return tuple(line.replace("$(ARCH)", arch).split()) + ("--cuda-device-only", "-S") + extra


@functools.lru_cache(maxsize=None)
def _compiler():
    return subprocess.run(["hipcc", "--version"], check=True, capture_output=True).stdout


def _key(unit, all_flags):
    h = hashlib.sha256("\0".join(all_flags).encode() + b"\0" + _compiler())
    headers = sorted(f for f in os.listdir(CSRC) if f.endswith((".h", ".hpp", ".inc")))
    for path in [os.path.join(CSRC, f) for f in [unit] + headers] + [os.path.join(ROOT, "include", "kzg_mi355x.h")]:
        h.update(open(path, "rb").read())
    return h.hexdigest()[:16]


@functools.lru_cache(maxsize=None)
def _artefact(unit, extra, remarks):
    """path of the cached assembly of `unit` (or, with `remarks`, of what the compiler wrote to stderr); compiles on a miss"""
    all_flags = flags(*extra)
    out = os.path.join(BUILD, "%s_%s.%s" % (unit.split(".")[0], _key(unit, all_flags), "txt" if remarks else "s"))
    if os.path.exists(out):
        return out
    os.makedirs(BUILD, exist_ok=True)
    tmp = "%s.%d.tmp" % (out, os.getpid())
    r = subprocess.run(["hipcc"] + list(all_flags) + [os.path.join(CSRC, unit), "-o", os.devnull if remarks else tmp],
                       capture_output=True, text=True)
    if r.returncode != 0:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise RuntimeError("hipcc failed on %s (exit status %d):\n%s" % (unit, r.returncode, r.stderr))
    if remarks:
        with open(tmp, "w") as f:
            f.write(r.stderr)
    os.replace(tmp, out)
    return out


def asm_path(unit, *extra):
    return _artefact(unit, extra, False)


def asm_text(unit, *extra):
    return open(asm_path(unit, *extra)).read()


def remarks_text(unit, *extra):
    """what the compiler says on stderr while it compiles `unit` with `extra` (-Rpass-analysis=... and the like)"""
    return open(_artefact(unit, extra, True)).read()


def kernel_meta(unit):
    """mangled kernel name -> every integer field of its block under amdhsa.kernels: (vgpr_count, vgpr_spill_count,
    sgpr_spill_count, private_segment_fixed_size, group_segment_fixed_size, ...); the fields of its arguments are not taken"""
    asm = asm_text(unit)
    meta = {}
    for block in asm[asm.index("amdhsa.kernels:"):asm.index("\namdhsa.target:")].split("\n  - .")[1:]:
        name = re.search(r"^    \.name:\s+(\S+)", block, re.M).group(1)
        meta[name] = {key: int(value) for key, value in re.findall(r"^(?:    \.)?(\w+):\s+(\d+)\s*$", block, re.M)}
    return meta
