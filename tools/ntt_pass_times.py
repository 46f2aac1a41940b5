"""Per-size pass times of k_ntt_pass from a rocprofv3 kernel trace (`rocprofv3 --kernel-trace --output-format csv`).

Every pass of a multi-pass transform of n = 2^k values launches n / 2048 workgroups (one 2048-value tile each), so the
grid identifies the size; single-pass transforms (n <= 2^11) are one workgroup.  Prints one JSON line per size: the
number of pass launches, the median and minimum pass time, and the median times the pass count of the plan
(engine.h: ntt_plan) as the kernel time of one direction.  Only passes that ran alone count: a launch that overlaps any
other kernel in time (the commitments-from-values leg of tests/perf_ntt.py runs beside the MSM) is left out.

usage: python tools/ntt_pass_times.py <kernel_trace.csv>
"""
import csv
import json
import sys


def passes(k):  # mirrors ntt_plan: one pass up to 2^11, then ceil(k / 9) passes
    return 1 if k <= 11 else (k + 8) // 9


def main(path):
    rows = list(csv.DictReader(open(path)))
    span = lambda r: (int(r["Start_Timestamp"]), int(r["End_Timestamp"]))  # noqa: E731
    others = sorted(span(r) for r in rows if "k_ntt_pass" not in r["Kernel_Name"])
    by_blocks = {}
    for r in rows:
        if "k_ntt_pass" not in r["Kernel_Name"]:
            continue
        t0, t1 = span(r)
        if any(a < t1 and t0 < b for a, b in others):
            continue
        blocks = int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])
        by_blocks.setdefault(blocks, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for blocks, t in sorted(by_blocks.items()):
        t.sort()
        k = (blocks * 2048).bit_length() - 1 if blocks > 1 else None
        row = {"log_n": k, "workgroups": blocks, "launches": len(t), "pass_median_us": round(t[len(t) // 2], 1),
               "pass_min_us": round(t[0], 1)}
        if k is not None:
            row["passes"] = passes(k)
            row["direction_kernels_us"] = round(row["pass_median_us"] * passes(k), 1)
        print(json.dumps(row))


if __name__ == "__main__":
    main(sys.argv[1])
