#!/bin/bash
# GPU box: the evidence of one round in one go.  usage: tools/round_profile.sh <tag>   (writes $PP_TOOL_OUT/<tag>_*, default tool_out/)
set -e
tag=$1
out=${PP_TOOL_OUT:-tool_out}
mkdir -p "$out"
python3 -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$out/${tag}_smoke.log" 2>&1
python3 bench.py --full > "$out/${tag}_bench.log" 2>&1
grep '^{' "$out/${tag}_bench.log" > "$out/${tag}_bench.json"
cd /tmp; export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
export PP_BENCH_PROFILED=1      # bench.py under rocprofv3: only the headline launches (no open-vertex run, no plan()-level legs)
rocprofv3 --kernel-trace --stats -d "$out/${tag}_prof" -o ${tag} --output-format csv -- python3 bench.py --full --no-cpu-baseline > "$out/${tag}_prof.log" 2>&1
grep '^{' "$out/${tag}_prof.log" > "$out/${tag}_bench_under_rocprof.json"
bash tools/traffic.sh > "$out/${tag}_traffic.log" 2>&1
echo done
