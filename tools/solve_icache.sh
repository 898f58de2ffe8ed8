#!/bin/bash
# GPU box: instruction-cache and instruction-fetch counters of pp_k_solve_edges on config 3, for prebuilt libraries
# build/libppgpu_<name>.so (profiles/solve_icache.txt).  Two counter passes per library, each a run of its own over three bench steps,
# counters only, the solve kernel's dispatches only:
#   SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQC_ICACHE_MISSES_DUPLICATE     requests of the instruction cache and what became of them
#   SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_IFETCH SQ_WAIT_INST_ANY SQ_INSTS_VALU   fetches issued, wave-cycles and those spent waiting for an instruction
# Every GPU step has a time limit of its own, and the script stops at the first that fails.  usage: tools/solve_icache.sh name [name ...]
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
[ $# -ge 1 ] || { echo "usage: tools/solve_icache.sh name [name ...]"; exit 2; }
out=${PP_TOOL_OUT:-tool_out}
export out
mkdir -p $out
export PP_BENCH_PROFILED=1
for n in "$@"; do
  [ -f build/libppgpu_$n.so ] || { echo "build/libppgpu_$n.so is missing"; exit 2; }
  export PPGPU_LIB_OVERRIDE=$PWD/build/libppgpu_$n.so
  pass=0
  for counters in "SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQC_ICACHE_MISSES_DUPLICATE" \
                  "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_IFETCH SQ_WAIT_INST_ANY SQ_INSTS_VALU"; do
    pass=$((pass + 1))
    rm -rf $out/icache_${n}_$pass
    timeout -k 10 300 rocprofv3 --pmc $counters --kernel-include-regex 'pp_k_solve_edges' --output-format csv -d $out/icache_${n}_$pass \
      -- python3 bench.py --steps 3 --warmup 1 --no-cpu-baseline > $out/icache_${n}_$pass.log 2>&1 \
      || { echo "counter pass $pass of $n failed (exit $?)"; tail -5 $out/icache_${n}_$pass.log; exit 1; }
  done
  python3 - $n <<'PY' || exit 1
import csv, glob, os, sys, collections
name = sys.argv[1]
tot, disp = collections.Counter(), collections.defaultdict(set)
for f in glob.glob(os.environ["out"] + f"/icache_{name}_*/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if r["Kernel_Name"].startswith("pp_k_solve_edges"):
            tot[r["Counter_Name"]] += float(r["Counter_Value"])
            disp[r["Counter_Name"]].add(r["Dispatch_Id"])
per = {k: tot[k] / max(1, len(disp[k])) for k in tot}
print(name, "pp_k_solve_edges, per dispatch:", " ".join("%s %.0f" % (k, v) for k, v in sorted(per.items())))
g = per.get
if g("SQC_ICACHE_REQ"):
    print(name, "  instruction cache: hit rate %.3f, misses per request %.3f (duplicates %.3f)" % (g("SQC_ICACHE_HITS", 0) / g("SQC_ICACHE_REQ"),
          g("SQC_ICACHE_MISSES", 0) / g("SQC_ICACHE_REQ"), g("SQC_ICACHE_MISSES_DUPLICATE", 0) / g("SQC_ICACHE_REQ")))
if g("SQ_WAVE_CYCLES"):
    print(name, "  share of wave-cycles waiting for an instruction %.3f; fetches per wave %.0f; VALU per wave %.0f" % (
          g("SQ_WAIT_INST_ANY", 0) / g("SQ_WAVE_CYCLES"), g("SQ_IFETCH", 0) / max(1, g("SQ_WAVES", 1)), g("SQ_INSTS_VALU", 0) / max(1, g("SQ_WAVES", 1))))
PY
done
