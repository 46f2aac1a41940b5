#!/bin/bash
# The front of the MSM pipeline (the sort kernels) against a library built from the parent commit, on ONE box in ONE go:
#   usage: tools/prof_sort_front.sh <parent libkzg_mi355x.so> [bench runs per side, default 4] [output directory, default prof_out/sort_front]
#   1. rocprofv3 --kernel-trace --stats of a short pipelined bench, parent          -> trace_parent/, front_parent.json, queues_parent.txt
#   2. the default bench.py --gpus 1 --no-cpu-baseline, parent and current alternating -> ab_bench.jsonl
#   3. the same trace with the current build                                          -> trace_current/, front_current.json, queues_current.txt
#   4. one commitment at a time (tools/prof_latency.py), both sides                  -> latency.jsonl
#   5. a counter-only pass each (no tracing beside it): executed VALU instructions of the recoding kernels -> pmc_valu_<side>/
#   and the summary of all of it                                                      -> sort_front.jsonl, sort_kernel_stats.csv
# Every step has its own time limit and the script stops at the first step that fails.
set -o pipefail
cd "$(dirname "$0")/.."
PARENT=$(readlink -f "$1")
RUNS=${2:-4}
[ -f "$PARENT" ] || { echo "usage: $0 <parent library> [runs] [output directory]"; exit 2; }
O=${3:-prof_out/sort_front}
mkdir -p $O
export TMPDIR=/tmp
BENCH="python3 bench.py --gpus 1 --no-cpu-baseline"
TRACED="python3 bench.py --no-cpu-baseline --no-extras --steps 16 --warmup 3"
SHORT="python3 bench.py --gpus 1 --steps 4 --warmup 1 --slots 1 --no-cpu-baseline --no-extras --no-openings"
step() {  # step <seconds> <log> <command...>
  local limit=$1 log=$2; shift 2
  timeout -k 10 $limit "$@" > $log 2>&1
  local rc=$?
  if [ $rc -ne 0 ]; then echo "STOP: rc=$rc in: $*"; tail -5 $log; exit $rc; fi
}
lib_of() { if [ $1 = parent ]; then echo $PARENT; else echo ""; fi; }
trace() {  # trace <side>
  rm -rf $O/trace_$1
  step 300 $O/trace_$1.log env KZG_MI355X_LIB=$(lib_of $1) rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_$1 -- $TRACED
  step 60 $O/queues_$1.txt python3 tools/stream_queues.py $O/trace_$1
  step 60 $O/front_$1.txt python3 tools/sort_front.py $O/trace_$1
  grep '^JSON ' $O/front_$1.txt | cut -c6- > $O/front_$1.json
  grep -E "^gaps in front|^front kernels" $O/queues_$1.txt
  grep -v "^k_sort_count:" $O/front_$1.txt | grep -v '^JSON ' | tail -2
}
trace parent
: > $O/ab_bench.jsonl
for i in $(seq 1 $RUNS); do
  for side in parent current; do
    step 300 $O/bench_${side}_$i.log env KZG_MI355X_LIB=$(lib_of $side) $BENCH
    tail -1 $O/bench_${side}_$i.log | python3 -c '
import json, sys
l = json.loads(sys.stdin.readline())
o = {"side": sys.argv[1], "run": int(sys.argv[2]), "value": l["value"], "ms_per_step": l["ms_per_step"],
     "avg_kernel_ms": l["roofline"]["avg_kernel_ms"], "step_minus_kernel_ms": l["ms_per_step"] - l["roofline"]["avg_kernel_ms"],
     "opening_proofs_per_sec": l["opening_proofs_per_sec"],
     "host_pointer_commitments_per_sec": l.get("host_pointer_commitments_per_sec"),
     "host_pointer_proofs_per_sec": l.get("host_pointer_proofs_per_sec"), "bit_exact_vs_golden": l["config"]["bit_exact_vs_golden"]}
print(json.dumps(o))' $side $i | tee -a $O/ab_bench.jsonl
  done
done
trace current
: > $O/latency.jsonl
for side in parent current; do
  step 200 $O/latency_$side.log env KZG_MI355X_LIB=$(lib_of $side) python3 tools/prof_latency.py 1048576 commit 20
  tail -1 $O/latency_$side.log | sed "s/^{/{\"side\": \"$side\", /" | tee -a $O/latency.jsonl
done
for side in parent current; do
  rm -rf $O/pmc_valu_$side
  step 300 $O/pmc_valu_$side.log env KZG_MI355X_LIB=$(lib_of $side) rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d $O/pmc_valu_$side -- $SHORT
done
python3 - $O <<'PY'
import csv, glob, json, re, statistics, sys
O = sys.argv[1]
SORT = ("k_sort_count", "k_sort_spread_staged", "k_sort_spread", "k_fine_count", "k_fine_binscan", "k_fine_scatter")
short = lambda name: (re.search(r"k_[a-z_0-9]+", name.split("(")[0]) or [name])[0]  # demangled or mangled
out = open(O + "/sort_front.jsonl", "w")
emit = lambda o: (out.write(json.dumps(o) + "\n"), print(json.dumps(o)))
# A/B
runs = [json.loads(l) for l in open(O + "/ab_bench.jsonl")]
ab = {"kind": "ab_summary"}
for key in ("value", "ms_per_step", "avg_kernel_ms", "step_minus_kernel_ms", "opening_proofs_per_sec", "host_pointer_commitments_per_sec",
            "host_pointer_proofs_per_sec"):
    ab[key] = {}
    for side in ("parent", "current"):
        v = [r[key] for r in runs if r["side"] == side and r[key] is not None]
        if v:
            ab[key][side] = {"min": min(v), "median": statistics.median(v), "max": max(v), "runs": v}
    if len(ab[key]) == 2:
        ab[key]["ratio_of_medians"] = ab[key]["current"]["median"] / ab[key]["parent"]["median"]
v = ab["value"]
ab["parent_spread_percent"] = 100.0 * (v["parent"]["max"] - v["parent"]["min"]) / v["parent"]["median"]
ab["slowest_current_beats_fastest_parent"] = v["current"]["min"] > v["parent"]["max"]
ab["bit_exact_vs_golden"] = all(r["bit_exact_vs_golden"] for r in runs)
for r in runs:
    emit(dict(r, kind="ab_run"))
emit(ab)
# traces
stats_rows = []
for side in ("parent", "current"):
    f = json.load(open("%s/front_%s.json" % (O, side)))
    f.pop("k_sort_count_launches")
    emit(dict(f, kind="trace", side=side))
    for p in glob.glob("%s/trace_%s/*/*kernel_stats.csv" % (O, side)):
        for r in csv.DictReader(open(p)):
            if short(r["Name"]) in SORT or short(r["Name"]) == "k_bucket_accumulate":
                stats_rows.append({"side": side, "kernel": short(r["Name"]), "name": r["Name"].split("(")[0], "calls": int(r["Calls"]),
                                   "average_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3})
with open(O + "/sort_kernel_stats.csv", "w") as fcsv:
    w = csv.DictWriter(fcsv, ["side", "kernel", "name", "calls", "average_us", "min_us", "max_us"])
    w.writeheader()
    w.writerows(stats_rows)
emit({"kind": "kernel_stats_pipelined_trace", "rows": stats_rows})
for l in open(O + "/latency.jsonl"):
    emit(dict(json.loads(l), kind="single_commitment_latency"))
# executed VALU instructions of the recoding kernels, per scalar of a 2^20 + 1 term commitment
for side in ("parent", "current"):
    per = {}
    for p in glob.glob("%s/pmc_valu_%s/*/*counter_collection.csv" % (O, side)):
        for r in csv.DictReader(open(p)):
            if r["Counter_Name"] == "SQ_INSTS_VALU" and short(r["Kernel_Name"]) in SORT[:3]:
                per.setdefault(short(r["Kernel_Name"]), []).append(float(r["Counter_Value"]))
    emit({"kind": "pmc_valu", "side": side,
          "SQ_INSTS_VALU_per_launch": {k: statistics.mean(v) for k, v in per.items()},
          "valu_instructions_per_scalar": {k: statistics.mean(v) * 64.0 / (1048576 + 1) for k, v in per.items()}})
out.close()
PY
