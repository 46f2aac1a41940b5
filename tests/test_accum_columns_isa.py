"""Every column of a Montgomery product in k_bucket_accumulate is ONE v_mad_i64_i32 chain that starts from the shifted carry
of the column below (field30.hip.h, KZG_F30_MAC): no chain opened from zero and joined with a 64-bit add, no second chain
subtracted with borrow in fq_mul_sub.  This test counts opcodes in the main loop of the compiler's output for gfx950 (the
assembly tests/test_accum_isa.py reads, from tests/isa_cache.py) and prices them with
tools/isa_histogram.py.  CPU only; it reads opcodes and counts, nothing else.

Before the change the loop held 3091 v_mad_i64_i32, 240 v_lshl_add_u64 (123 joins, 111 rounding adds, 6 others), 25 + 25
v_sub_co_u32 / v_subb_co_u32, 74 s_nop (78 in the whole kernel) and 7530 priced issue units
(profiles/r16_accum_isa_histogram.txt).

The units: the joins (123 x 1.69 = 208) and the subtract pairs (74, less the 13 negations that replace them) are gone, 267
units.  The 300 the change set out for counted 77 more from taking the rounding half 2^29 out of the upper columns, and that
part did NOT yield: once a column is a single chain from the carry there is no chain left whose initial addend could carry
the bias for nothing, so a biased accumulator needs its 2^29 added every column just the same (and then an xor in front of
the digit on top); a bias of 2^29 + 2^59 that survives the shift does not fit the 0.45 x 2^60 the column bound leaves.  What
stands is one 64-bit add per upper column and none per lower one.  The threshold below is what was reached."""
import collections
import os
import re
import subprocess
import sys

from isa_cache import ROOT, asm_path, requires_hipcc
from test_accum_isa import UNIT

RATES = os.path.join(ROOT, "profiles", "r03_instr_rates.jsonl")
TOOL = os.path.join(ROOT, "tools", "isa_histogram.py")

PARENT_UNITS = 7530
PARENT_NOP_LOOP, PARENT_NOP_KERNEL = 74, 78
REACHED = 267  # priced units below the parent (see above; 300 with the rounding adds gone)

pytestmark = requires_hipcc


def main_loop_opcodes():
    """opcodes of the kernel's main loop, found the way tools/isa_histogram.py finds it: from the loop header in front of
    the LDS-DMA gathers to the last block that belongs to that loop"""
    asm = open(asm_path(UNIT)).read().splitlines()
    start = next(i for i, l in enumerate(asm) if re.match(r"^_ZN3kzg19k_bucket_accumulate.*:\s*; @", l))
    end = next(i for i in range(start, len(asm)) if "s_endpgm" in asm[i])
    body = asm[start:end]
    heads = [i for i, l in enumerate(body) if "Loop Header: Depth=1" in l]
    dma = [i for i, l in enumerate(body) if "global_load_lds_dwordx4" in l]
    head = max(h for h in heads if h < dma[-1])
    name = body[head].split(":")[0].strip().lstrip(".L")
    labels = [i for i, l in enumerate(body) if re.match(r"^\.LBB\d+_\d+:", l)]
    inside = [i for i in labels if ("Header=%s " % name) in body[i] + " " or ("Parent Loop %s " % name) in body[i] + " "]
    first = min([head] + inside)
    after = [i for i in labels if i > max(inside) and i not in inside]
    last = (after[0] if after else len(body)) - 1
    loop = [l.split()[0] for l in body[first:last + 1] if l.startswith("\t") and not l.strip().startswith((";", "."))]
    kernel = [l.split()[0] for l in body if l.startswith("\t") and not l.strip().startswith((";", "."))]
    return collections.Counter(loop), collections.Counter(kernel)


def count(hist, op):
    return sum(n for k, n in hist.items() if k == op or k in (op + "_e32", op + "_e64"))


def test_one_chain_per_column_in_the_main_loop():
    loop, kernel = main_loop_opcodes()
    figures = {op: count(loop, op) for op in ("v_mad_i64_i32", "v_lshl_add_u64", "v_sub_co_u32", "v_subb_co_u32", "s_nop")}
    print("main loop:", figures, "whole kernel s_nop:", count(kernel, "s_nop"))
    assert figures["v_mad_i64_i32"] <= 3091
    assert figures["v_lshl_add_u64"] <= 120  # one rounding add per upper column; no joins
    assert figures["v_sub_co_u32"] + figures["v_subb_co_u32"] == 0
    assert figures["s_nop"] <= PARENT_NOP_LOOP + 30
    assert count(kernel, "s_nop") <= PARENT_NOP_KERNEL + 30


def test_priced_issue_units_of_the_main_loop():
    out = subprocess.run([sys.executable, TOOL, asm_path(UNIT), RATES], check=True, capture_output=True, text=True).stdout
    m = re.search(r"multiply-adds: (\d+) of (\d+) units", out)
    assert m, out
    mads, units = int(m.group(1)), int(m.group(2))
    print("priced units: %d (multiply-adds %d), parent %d" % (units, mads, PARENT_UNITS))
    assert units <= PARENT_UNITS - REACHED
