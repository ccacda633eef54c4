#!/bin/bash
# Run on the GPU box.  A/B of two BUILT trees of this repository on one box in one job: this tree against another one
# (the parent commit, exported and built beside it), for a change to a kernel that is not an experiment registration.
#  1. plain `python bench.py`, alternating other, this, ... N times each (default 4);
#  2. one `python bench.py --full --no-cpu-baseline` per tree (verified, the legs);
#  3. both trees under rocprofv3: --kernel-trace --stats in one run, the SQ instruction counts and the SQ wave cycles
#     in a run of their own each (counters never together with a trace).
# Every GPU step has its own time limit and the steps are chained: the first failure ends the job.
# Output: <out>/ab.txt (one line per bench run), <out>/prof/{other,this}_{stats,sq,sqwait}/ for
# tools/summarize_two_trees.py.   -> profiles/r05_packed_rows.txt
# usage: tools/ab_two_trees.sh <other tree> [runs] [out dir]
set -o pipefail
THIS="$(cd "$(dirname "$0")/.." && pwd)"
OTHER="$(cd "${1:?usage: tools/ab_two_trees.sh <other tree> [runs] [out dir]}" && pwd)"
RUNS="${2:-4}"
OUT="${3:-$THIS/build/ab_two_trees}"
mkdir -p "$OUT/prof"
: > "$OUT/ab.txt"

bench() { # tree tag limit args...
    local tree="$1" tag="$2" limit="$3"
    shift 3
    (cd "$tree" && timeout -k 10 "$limit" python3 bench.py "$@" 2> "$OUT/$tag.err" | tail -n 1 > "$OUT/$tag.json") || return 1
    python3 -c '
import json, sys
d = json.loads(open(sys.argv[1]).read())
out = {k: d.get(k) for k in ("value", "ms_per_step", "verified")}
for name, leg in (d.get("legs") or {}).items():
    if isinstance(leg, dict):
        out[name] = {k: leg[k] for k in ("value", "verified") if k in leg}
print(sys.argv[2], json.dumps(out))' "$OUT/$tag.json" "$tag" >> "$OUT/ab.txt" || return 1
    tail -n 1 "$OUT/ab.txt" | cut -c 1-300
}

profile() { # tree tag
    local tree="$1" tag="$2" p="$OUT/prof"
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$p/${tag}_stats" -- \
        python3 "$tree/bench.py" --gpus 1 --steps 5 --warmup 2 > "$p/${tag}_stats.log" 2> "$p/${tag}_stats.err" || return 1
    timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVES SQ_INSTS_LDS --output-format csv -d "$p/${tag}_sq" -- \
        python3 "$tree/bench.py" --gpus 1 --steps 2 --warmup 1 > "$p/${tag}_sq.log" 2> "$p/${tag}_sq.err" || return 1
    timeout -k 10 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU \
        --output-format csv -d "$p/${tag}_sqwait" -- \
        python3 "$tree/bench.py" --gpus 1 --steps 2 --warmup 1 > "$p/${tag}_sqwait.log" 2> "$p/${tag}_sqwait.err" || return 1
    echo "$tag profiled"
}

for i in $(seq 1 "$RUNS"); do
    bench "$OTHER" "other$i" 240 && bench "$THIS" "this$i" 240 || exit 1
done
bench "$OTHER" other_full 600 --full --no-cpu-baseline && bench "$THIS" this_full 600 --full --no-cpu-baseline || exit 1
cd /tmp && export TMPDIR=/tmp
profile "$OTHER" other && profile "$THIS" this || exit 1
# (the raw traces can be large; the stats and the counter tables are what the summary reads)
find "$OUT/prof" -name "*.csv" -size +6M -delete
