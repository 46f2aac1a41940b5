"""CPU: the extent check of include/kzg_mi355x.hpp under host sanitizers.

tests/hpp/hpp_extents.cpp calls every wrapper of the header over tests/hpp/abi_extent_stub.cpp, a stand-in for the C-ABI that
reads every documented input byte and writes every documented output byte of each call.  The two are compiled into ONE
stand-alone program with AddressSanitizer and UBSan, their runtimes linked statically, and run directly in the environment as it
is: the test preloads nothing, nothing is loaded into Python, no device and no libkzg_mi355x.so are involved.  A buffer the
header sizes one element short, a wrong stride or count, a handle destroyed twice or used after its destruction ends the program
with a sanitizer report; the program itself checks the size of every returned container and that the header's own size checks
throw before the library is called."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HPP = os.path.join(ROOT, "include", "kzg_mi355x.hpp")
SRC = [os.path.join(ROOT, "tests", "hpp", f) for f in ("abi_extent_stub.cpp", "hpp_extents.cpp")]
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D_GLIBCXX_ASSERTIONS",
         "-I" + os.path.join(ROOT, "include")]


def _compilers():
    """g++ first; a clang++ of the path or of the ROCm installation where g++ has no sanitizer runtime"""
    out = [shutil.which("g++"), shutil.which("clang++")]
    for rocm in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if rocm:
            out.append(os.path.join(rocm, "llvm", "bin", "clang++"))
    return [c for c in out if c and os.path.exists(c)]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """(the program, the same with one direct call to a stub made one element short), built once"""
    d = tmp_path_factory.mktemp("hpp_extents")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    tried = []
    for cxx in _compilers():
        # the sanitizer runtimes are linked statically (clang does so by default): the program then starts the same way whatever
        # the environment it inherits preloads, and the runtime's link-order check has nothing to object to
        static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
        r = subprocess.run([cxx] + FLAGS + static + [str(probe), "-o", str(d / "probe")], capture_output=True, text=True)
        tried.append((cxx, r.stderr[-300:]))
        if r.returncode == 0:
            break
    else:
        pytest.fail("no C++ compiler with an AddressSanitizer runtime: %r" % (tried,))
    # the stub once, the program twice, side by side; then two links
    jobs = [[cxx] + FLAGS + ["-c", SRC[0], "-o", str(d / "stub.o")],
            [cxx] + FLAGS + ["-c", SRC[1], "-o", str(d / "full.o")],
            [cxx] + FLAGS + ["-DHPP_EXTENTS_SHORT", "-c", SRC[1], "-o", str(d / "short.o")]]
    procs = [subprocess.Popen(j, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for j in jobs]
    for j, p in zip(jobs, procs):
        out, _ = p.communicate(timeout=600)
        assert p.returncode == 0, (j, out[-3000:])
    exes = []
    for name in ("full", "short"):
        exe = str(d / ("hpp_extents_" + name))
        r = subprocess.run([cxx] + FLAGS + static + [str(d / "stub.o"), str(d / (name + ".o")), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        exes.append(exe)
    return exes


def _run(exe):
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}  # the sanitizers' defaults
    return subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)


def _symbols_the_header_calls():
    text = re.sub(r"//[^\n]*", "", open(HPP).read())  # the comments name calls the header does not make
    return set(re.findall(r"\b(kzg_[a-z0-9_]+)\s*\(", text))


def test_every_wrapper_stays_inside_its_buffers(programs):
    """the sanitizer build runs clean: every extent the header computes covers what the C header documents"""
    r = _run(programs[0])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "hpp_extents ok" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]


def test_every_symbol_the_header_calls_is_exercised(programs):
    """the kzg_* calls in the header's text == the stubs the program reached: a wrapper added without a case fails here"""
    r = _run(programs[0])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    seen = {m.group(1) for m in re.finditer(r"^called (kzg_[a-z0-9_]+) (\d+)$", r.stdout, re.M) if int(m.group(2)) > 0}
    called = _symbols_the_header_calls()
    assert len(called) > 50, "the regular expression lost the header's calls"
    assert called == seen, {"not exercised": sorted(called - seen), "not in the header": sorted(seen - called)}


def test_stub_defines_what_the_header_calls():
    """every symbol the header calls has a stub with the C header's prototype (the stub includes kzg_mi355x.h, so a drift does
    not compile); here: none is missing from the stub's text, so the link cannot quietly pick up a real library"""
    stub = open(SRC[0]).read()
    missing = [s for s in sorted(_symbols_the_header_calls()) if not re.search(r"^[a-z_ \*]+\b%s\(" % s, stub, re.M)]
    assert not missing, missing


def test_a_short_buffer_is_reported(programs):
    """the harness can fail: one of the program's own direct calls to a stub gets a vector one element short"""
    r = _run(programs[1])
    assert r.returncode != 0
    assert "AddressSanitizer: heap-buffer-overflow" in r.stderr, r.stderr[-3000:]
    assert "kzg_srs_read_g1" in r.stderr
    assert "hpp_extents ok" not in r.stdout
