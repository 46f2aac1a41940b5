"""The accumulation kernel waits for "all but the youngest 17" vector-memory operations after a bucket flush
(msm_accum.hip, accum_take_point): that is only correct while the flush path issues AT LEAST 17 such operations between the
gather of the point and the wait.  This test counts them in the compiler's output for gfx950.  CPU only (hipcc cross-compiles);
the assembly comes from tests/isa_cache.py."""
import re

from isa_cache import asm_text, requires_hipcc

UNIT = "msm_accum.hip"


def kernel_asm():
    asm = asm_text(UNIT)
    i = asm.index("_ZN3kzg19k_bucket_accumulateE")
    i = asm.index(":", i)
    return asm[i:asm.index(".end_amdhsa_kernel", i)].splitlines(), asm


def is_vmem(line):
    op = line.split()[0] if line.split() else ""
    return op.startswith(("global_load", "global_store", "global_atomic", "scratch_", "buffer_", "flat_"))


@requires_hipcc
def test_flush_path_issues_the_operations_the_partial_wait_counts():
    body, _ = kernel_asm()
    waits = [n for n, l in enumerate(body) if re.search(r"s_waitcnt\s+vmcnt\(17\)", l)]
    assert len(waits) == 1, "one partial wait, in accum_take_point"
    w = waits[0]
    # walk back to the flush: the asm block of sixteen 16-byte stores
    stores = [n for n in range(w) if "global_store_dwordx4" in body[n]]
    first = max(n for n in stores if not any(m for m in stores if m == n - 1))  # start of the last run of consecutive stores
    run = [n for n in stores if n >= first]
    assert len(run) == 16 and run == list(range(first, first + 16)), "sixteen consecutive stores"
    # between the stores and the wait: the walk over empty buckets (a loop that waits for everything itself) and exactly one
    # more load on the straight path; nothing else that touches vector memory
    tail = [l for l in body[first + 16:w] if l.startswith("\t") and is_vmem(l.strip())]
    straight = [l for l in tail if "global_load_dword " in l or "global_load_dword\t" in l]
    assert all("global_load_dword" in l for l in tail), tail
    assert 1 <= len(straight) <= 2, tail  # the load inside the walk loop and the one behind it
    loop_waits = [n for n in range(first + 16, w) if re.search(r"s_waitcnt\s+vmcnt\(0\)", body[n])]
    assert len(tail) == 1 or loop_waits, "a second load is only allowed inside the walk, which waits for everything"


def test_two_workgroups_per_cu_by_register_count():
    body, asm = kernel_asm()
    body_text = "\n".join(body)
    i = asm.index(".name:           _ZN3kzg19k_bucket_accumulateE")
    m = re.search(r"\.vgpr_count:\s+(\d+)", asm[i:i + 2000])
    v = int(m.group(1))
    assert 169 <= v <= 256, "three workgroups of this kernel must not fit a CU (see the comment at its top): %d VGPRs" % v
    assert "s_waitcnt vmcnt(17)" in body_text
