#!/usr/bin/env python3
"""Where the first kernel of every MSM job started, from a rocprofv3 --kernel-trace csv of bench.py: for every k_sort_count of
the pipelined part, its start relative to the nearest accumulation boundary (the end of one k_bucket_accumulate / the start of
the next), whether it started INSIDE a running accumulation (it can only if it fits on a CU beside two accumulation workgroups:
msm_sort.hip, at kRecodeBlock) and its duration; the durations of the five sort kernels over the same part; the gaps in front of
the accumulations.
usage: sort_front.py <kernel_trace.csv | directory holding one> [first accumulation, default 8]"""
import csv, glob, json, os, re, statistics, sys

SORT = ("k_sort_count", "k_sort_spread", "k_sort_spread_staged", "k_fine_count", "k_fine_binscan", "k_fine_scatter")


def summary(v):
    v = sorted(v)
    return {"n": len(v), "min": v[0], "median": statistics.median(v), "mean": statistics.mean(v), "max": v[-1]} if v else {"n": 0}


def main():
    path = sys.argv[1]
    if os.path.isdir(path):
        path = sorted(glob.glob(path + "/**/*kernel_trace.csv", recursive=True))[-1]
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                 (re.search(r"k_[a-z_0-9]+", r["Kernel_Name"].split("(")[0]) or [r["Kernel_Name"]])[0]) for r in csv.DictReader(open(path)))
    acc = [e for e in ev if e[2] == "k_bucket_accumulate"]
    acc = acc[min(first, len(acc) - 1):]
    t_from, t_to = acc[0][0], acc[-1][1]
    bounds = sorted([a[0] for a in acc] + [a[1] for a in acc])
    rows = []
    for s, e, name in ev:
        if name != "k_sort_count" or s < t_from or s > t_to:
            continue
        running = [a for a in acc if a[0] <= s < a[1]]
        near = min(bounds, key=lambda b: abs(b - s))
        rows.append({"start_minus_nearest_boundary_us": (s - near) / 1e3, "duration_us": (e - s) / 1e3,
                     "inside_accumulation": bool(running),
                     "into_accumulation": (s - running[0][0]) / (running[0][1] - running[0][0]) if running else None})
    # "inside" proper: further than 20 us from either end of the accumulation it started in
    deep = [r for r in rows if r["inside_accumulation"] and abs(r["start_minus_nearest_boundary_us"]) > 20.0]
    gaps = [(b[0] - a[1]) / 1e3 for a, b in zip(acc, acc[1:])]
    kernels = {}
    for s, e, name in ev:
        if name in SORT and t_from <= s <= t_to:
            kernels.setdefault(name, []).append((e - s) / 1e3)
    out = {"trace": os.path.basename(path), "accumulations": len(acc),
           "accumulation_us": summary([(a[1] - a[0]) / 1e3 for a in acc]),
           "period_us": (acc[-1][0] - acc[0][0]) / 1e3 / max(1, len(acc) - 1),
           "gap_in_front_of_accumulation_us": summary(gaps),
           "k_sort_count": {"launches": len(rows), "started_inside_an_accumulation": sum(r["inside_accumulation"] for r in rows),
                            "started_more_than_20us_from_its_ends": len(deep),
                            "abs_start_minus_nearest_boundary_us": summary([abs(r["start_minus_nearest_boundary_us"]) for r in rows]),
                            "duration_us": summary([r["duration_us"] for r in rows])},
           "sort_kernels_us": {k: summary(v) for k, v in sorted(kernels.items())},
           "k_sort_count_launches": rows}
    for r in rows:
        print("k_sort_count: start %+8.1f us from the nearest boundary, %s, ran %7.1f us"
              % (r["start_minus_nearest_boundary_us"],
                 "inside an accumulation (%.0f %% in)" % (100 * r["into_accumulation"]) if r["inside_accumulation"] else "between accumulations",
                 r["duration_us"]))
    print("gaps us:", [round(g) for g in gaps])
    print("JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
