#!/bin/bash
# GPU box: A/B of prebuilt libraries build/libppgpu_<name>.so on one box: rocprofv3 kernel averages of a short bench run, alternating
# A B A B ... (`alternations` runs of each, 2 by default), then per figure each library's mean and spread (max - min) and whether
# B's mean lies within A's mean + A's spread, and the records hash of both.  Every GPU step has a time limit of its own, and the
# script stops at the first step that fails.  Logs and profiles go under $PP_TOOL_OUT (default tool_out/).  usage: tools/ab_libs.sh nameA nameB [alternations]
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
A=$1; B=$2; N=${3:-2}
[ -n "$A" ] && [ -n "$B" ] && [ "$N" -ge 1 ] || { echo "usage: tools/ab_libs.sh nameA nameB [alternations]"; exit 2; }
for n in $A $B; do [ -f build/libppgpu_$n.so ] || { echo "build/libppgpu_$n.so is missing"; exit 2; }; done
export PP_BENCH_PROFILED=1
out=${PP_TOOL_OUT:-tool_out}       # where the profiles and logs go
export out
mkdir -p $out
: > $out/ab_runs.jsonl
for ((i = 0; i < N; i++)); do
  for n in $A $B; do
    export PPGPU_LIB_OVERRIDE=$PWD/build/libppgpu_$n.so
    rm -rf $out/ab_$n
    # (13 steps of config 3 and the workload's set-up, under the tracer: a minute or two)
    timeout -k 10 420 rocprofv3 --kernel-trace --stats -d $out/ab_$n -o v --output-format csv -- python3 bench.py --no-cpu-baseline --steps 10 --warmup 3 > $out/ab_$n.log 2>&1 \
      || { echo "bench run of $n failed (exit $?)"; tail -5 $out/ab_$n.log; exit 1; }
    python3 - $n <<'PY' || exit 1
import csv,sys,json,os
rows=list(csv.DictReader(open(os.environ["out"]+f"/ab_{sys.argv[1]}/v_kernel_stats.csv")))
d={r['Name'].split('(')[0]:float(r['AverageNs'])/1e3 for r in rows}
ms=[json.loads(l)['ms_per_step'] for l in open(os.environ["out"]+f"/ab_{sys.argv[1]}.log") if l.startswith('{')]
run={k:round(d[k],1) for k in ('pp_k_cover_sweep','pp_k_pose_sweep','pp_k_plan_skips','pp_k_approach_events','pp_k_cover_finish')}
# the head of a launch (profiles/solve_icache.txt): the solve, the marking, the fan-out, and the table's reset where a library still has one
run.update({k:round(d.get(k,0.0),1) for k in ('pp_k_solve_edges','pp_k_mark_sweeps','pp_k_share_fanout')})
# shared tracks (profiles/arc_stops.txt): the members' copy per launch, and the arc walk, which a run's first launch alone queues
run.update({k:round(d.get(k,0.0),1) for k in ('pp_k_track_fanout','pp_k_arc_stops')})
run['fill']=round(sum(v for k,v in d.items() if 'fillBuffer' in k),1)
run['solve+mark+fanout+fill']=round(run['pp_k_solve_edges']+run['pp_k_mark_sweeps']+run['pp_k_share_fanout']+run['fill'],1)
print(sys.argv[1], run, 'ms_per_step', ms)
run['ms_per_step']=ms[-1]
open(os.environ["out"]+"/ab_runs.jsonl","a").write(json.dumps({"lib":sys.argv[1],"run":run})+"\n")
PY
  done
done
python3 - $A $B <<'PY'
import sys,json,os
runs=[json.loads(l) for l in open(os.environ["out"]+"/ab_runs.jsonl")]
a,b=([r["run"] for r in runs if r["lib"]==n] for n in sys.argv[1:3])
for k in a[0]:
    va,vb=[r[k] for r in a],[r[k] for r in b]
    ma,mb,sa,sb=sum(va)/len(va),sum(vb)/len(vb),max(va)-min(va),max(vb)-min(vb)
    print("%-22s %s mean %.4g spread %.3g   %s mean %.4g spread %.3g   %s" % (k, sys.argv[1], ma, sa, sys.argv[2], mb, sb, "within" if mb <= ma + sa else "BEYOND"))
PY
for n in $A $B; do
  PPGPU_LIB_OVERRIDE=$PWD/build/libppgpu_$n.so timeout -k 10 240 python3 tools/records_hash.py | grep -v amdgpu || { echo "records hash of $n failed"; exit 1; }
done
