#!/bin/bash
# A/B of the accumulation kernel against a library built from the parent commit, on ONE box in ONE go:
#   usage: tools/prof_accum_ab.sh <parent libkzg_mi355x.so> [bench runs per side, default 4] [output directory, default prof_out/accum_ab]
#   1. bench.py --gpus 1 --no-extras --no-cpu-baseline, parent and current alternating        -> ab_bench.jsonl
#   2. rocprofv3 --kernel-trace --stats on single commitments at 2^20 (tools/prof_latency.py)  -> ab_kernel_stats.json
#   3. counter-only passes (no tracing beside them): executed VALU instructions of the kernel, both sides; VALU busy figures and
#      HBM traffic of the current build                                                        -> ab_pmc.json
# AB_BENCH="python3 bench.py --gpus 1 --no-cpu-baseline" runs the default bench (extras included) in step 1; AB_CURRENT_PMC=0 leaves
# out the busy and traffic counters of the current build in step 3.
# Every step has its own time limit and the script stops at the first step that fails.
set -o pipefail
cd "$(dirname "$0")/.."
PARENT=$(readlink -f "$1")
RUNS=${2:-4}
[ -f "$PARENT" ] || { echo "usage: $0 <parent library> [runs] [output directory]"; exit 2; }
O=${3:-prof_out/accum_ab}
mkdir -p $O
export TMPDIR=/tmp
BENCH=${AB_BENCH:-"python3 bench.py --gpus 1 --no-extras --no-cpu-baseline"}
SHORT="python3 bench.py --gpus 1 --steps 4 --warmup 1 --slots 1 --no-cpu-baseline --no-extras --no-openings"
: > $O/ab_bench.jsonl
step() {  # step <seconds> <log> <command...>
  local limit=$1 log=$2; shift 2
  timeout -k 10 $limit "$@" > $log 2>&1
  local rc=$?
  if [ $rc -ne 0 ]; then echo "STOP: rc=$rc in: $*"; tail -5 $log; exit $rc; fi
}
for i in $(seq 1 $RUNS); do
  for side in parent current; do
    if [ $side = parent ]; then lib=$PARENT; else lib=""; fi
    step 300 $O/bench_${side}_$i.log env KZG_MI355X_LIB=$lib $BENCH
    tail -1 $O/bench_${side}_$i.log | python3 -c '
import json, sys
l = json.loads(sys.stdin.readline())
o = {"side": sys.argv[1], "run": int(sys.argv[2]), "value": l["value"], "ms_per_step": l["ms_per_step"], "avg_kernel_ms": l["roofline"]["avg_kernel_ms"],
     "mixed_additions_per_launch": l["valu"]["mixed_additions_per_launch"], "bit_exact_vs_golden": l["config"].get("bit_exact_vs_golden", l.get("bit_exact_vs_golden"))}
print(json.dumps(o))' $side $i | tee -a $O/ab_bench.jsonl
  done
done
for side in parent current; do
  if [ $side = parent ]; then lib=$PARENT; else lib=""; fi
  rm -rf $O/st_$side
  step 300 $O/st_$side.log env KZG_MI355X_LIB=$lib rocprofv3 --kernel-trace --stats --output-format csv -d $O/st_$side -- python3 tools/prof_latency.py 1048576 commit 10
  rm -rf $O/pmc_valu_$side
  step 300 $O/pmc_valu_$side.log env KZG_MI355X_LIB=$lib rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES --output-format csv -d $O/pmc_valu_$side -- $SHORT
done
i=0
[ "${AB_CURRENT_PMC:-1}" = 0 ] ||
for grp in "GRBM_GUI_ACTIVE GRBM_COUNT" "VALUBusy" "VALUUtilization" "FETCH_SIZE" "WRITE_SIZE" "TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum TCC_HIT_sum TCC_MISS_sum"; do
  i=$((i+1)); rm -rf $O/pmc_cur_$i
  step 300 $O/pmc_cur_$i.log rocprofv3 --pmc $grp --output-format csv -d $O/pmc_cur_$i -- $SHORT
done
python3 - $O <<'PY'
import csv, glob, json, sys
O = sys.argv[1]
stats = {}
for side in ("parent", "current"):
    for f in glob.glob("%s/st_%s/*/*kernel_stats.csv" % (O, side)):
        for r in csv.DictReader(open(f)):
            stats.setdefault(side, {})[r["Name"].split("(")[0]] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3}
json.dump(stats, open(O + "/ab_kernel_stats.json", "w"), indent=1)
def counters(pattern):
    res = {}
    for f in glob.glob(pattern):
        for r in csv.DictReader(open(f)):
            if "k_bucket_accumulate" in r["Kernel_Name"] and "pairs" not in r["Kernel_Name"]:
                res.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    return {k: sum(v) / len(v) for k, v in res.items()}
pmc = {"parent": counters(O + "/pmc_valu_parent/*/*counter_collection.csv"),
       "current": counters(O + "/pmc_valu_current/*/*counter_collection.csv")}
pmc["current"].update(counters(O + "/pmc_cur_*/*/*counter_collection.csv"))
madds = json.loads(open(O + "/ab_bench.jsonl").readline())["mixed_additions_per_launch"]
for side in ("parent", "current"):
    if "SQ_INSTS_VALU" in pmc[side]:
        pmc[side]["valu_instructions_per_mixed_addition"] = pmc[side]["SQ_INSTS_VALU"] / (madds / 64.0)
pmc["mixed_additions_per_launch"] = madds
json.dump(pmc, open(O + "/ab_pmc.json", "w"), indent=1)
for side in ("parent", "current"):
    a = stats.get(side, {}).get("kzg::k_bucket_accumulate", stats.get(side, {}))
    print(side, "k_bucket_accumulate", a if "avg_us" in a else "", "VALU/madd", pmc[side].get("valu_instructions_per_mixed_addition"))
PY
