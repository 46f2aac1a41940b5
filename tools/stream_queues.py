#!/usr/bin/env python3
"""Where the MSM pipeline's kernels ran, from a rocprofv3 --kernel-trace csv of bench.py:
  1. the hardware queue of every phase (front: sort and quotient kernels; accumulation; tail: finalisation and tree sums)
     and, where the trace has a stream column, the streams seen in every queue -- streams that share a queue are listed
     together;
  2. the gap in front of every k_bucket_accumulate (previous accumulation's end to this one's start), and what ran in it;
  3. how many front kernels directly follow a tail kernel in their hardware queue: there the next job's sort can stand
     behind a tail that is still waiting for its accumulation (the effect DESIGN.md section 5.0n removes; 0 when the front
     and tail streams have queues of their own).
usage: stream_queues.py <kernel_trace.csv | directory holding one> [first accumulation, default 8] [accumulations, default 24]"""
import csv, glob, json, os, statistics, sys

FRONT = ("k_sort_", "k_fine_", "k_poly_", "k_points_", "k_sets_", "k_tail_nonzero", "k_combine")
TAIL = ("k_bucket_finalize", "k_heavy_tree", "k_tree_sum")


def phase(name):
    if name == "k_bucket_accumulate":
        return "accum"
    if name.startswith(TAIL):
        return "tail"
    if name.startswith(FRONT):
        return "front"
    return "other"


def main():
    path = sys.argv[1]
    if os.path.isdir(path):
        path = sorted(glob.glob(path + "/**/*kernel_trace.csv", recursive=True))[-1]
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    count = int(sys.argv[3]) if len(sys.argv) > 3 else 24
    rows = list(csv.DictReader(open(path)))
    has_stream = "Stream_Id" in rows[0]
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                 r["Kernel_Name"].split("(")[0].split("::")[-1].replace("void ", "").split("<")[0], r.get("Queue_Id", "?"),
                 r.get("Stream_Id", "?")) for r in rows)
    acc = [e for e in ev if e[2] == "k_bucket_accumulate"]
    out = {"trace": os.path.basename(path), "accumulations": len(acc)}
    # 1. queues per phase, streams per queue (over the pipelined part only: from the first-th accumulation on)
    t_from = acc[min(first, len(acc) - 1)][0]
    queues, streams = {}, {}
    for e in ev:
        if e[0] < t_from:
            continue
        p = phase(e[2])
        queues.setdefault(p, {}).setdefault(e[3], 0)
        queues[p][e[3]] += 1
        if has_stream:
            streams.setdefault(e[3], {}).setdefault(e[4], set()).add(p)
    out["kernels_per_phase_and_queue"] = queues
    if has_stream:
        out["streams_per_queue"] = {q: {s: sorted(ps) for s, ps in ss.items()} for q, ss in streams.items()}
    print("phase -> queue: kernels", json.dumps(queues))
    if has_stream:
        for q, ss in sorted(streams.items()):
            print("queue %s carries streams %s" % (q, ", ".join("%s (%s)" % (s, "+".join(sorted(ps))) for s, ps in sorted(ss.items()))))
    # 2. gaps
    sel = acc[first:first + count + 1]
    gaps = []
    for a, b in zip(sel, sel[1:]):
        inside = [e for e in ev if e[1] > a[1] and e[0] < b[0] and e[2] != "k_bucket_accumulate"]
        gaps.append({"gap_us": (b[0] - a[1]) / 1e3, "accum_us": (b[1] - b[0]) / 1e3,
                     "in_gap": [{"kernel": e[2], "queue": e[3], "stream": e[4], "from_us": (e[0] - a[1]) / 1e3, "to_us": (e[1] - a[1]) / 1e3}
                                for e in inside]})
    g = [x["gap_us"] for x in gaps]
    if g:
        period = (sel[-1][0] - sel[0][0]) / 1e3 / (len(sel) - 1)
        out["gap_us"] = {"n": len(g), "mean": statistics.mean(g), "median": statistics.median(g), "min": min(g), "max": max(g)}
        out["accum_us_mean"] = statistics.mean(x["accum_us"] for x in gaps)
        out["period_us"] = period
        print("gaps in front of %d accumulations (us): mean %.0f median %.0f min %.0f max %.0f; kernel mean %.0f; period %.0f"
              % (len(g), out["gap_us"]["mean"], out["gap_us"]["median"], min(g), max(g), out["accum_us_mean"], period))
        print("gaps us:", [round(x) for x in g])
        for x in gaps[:4]:
            print("  gap %.0f us:" % x["gap_us"])
            for k in x["in_gap"]:
                print("    q%-3s s%-3s %7.0f .. %7.0f  %s" % (k["queue"], k["stream"], k["from_us"], k["to_us"], k["kernel"]))
    # 3. front kernels whose predecessor in their queue is a tail kernel
    by_q = {}
    for e in ev:
        if e[0] >= t_from:
            by_q.setdefault(e[3], []).append(e)
    behind = 0
    for q, es in by_q.items():
        for a, b in zip(es, es[1:]):
            if phase(a[2]) == "tail" and phase(b[2]) == "front":
                behind += 1
    out["front_kernels_directly_behind_a_tail_in_their_queue"] = behind
    print("front kernels that follow a tail kernel in their queue:", behind)
    print("JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
