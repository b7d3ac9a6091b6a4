#!/bin/bash
# rocprofv3 --kernel-trace --stats of one plain bench.py run (nothing else traced), condensed: the average time of every kernel of the
# timed steps, how much of each pyramid-levels dispatch ran inside the interval of a motion-search / transform dispatch, and the
# timeline of the last three steps.  For the A/B of the co-run order (profiles/ab_pyramid_beside_search.txt).
# usage: tools/trace_overlap.sh <out.txt> [root of the build to trace = this checkout] [bench args...]
set -u
here=$(cd "$(dirname "$0")/.." && pwd)
out=$(realpath -m "$1"); shift
root=$here
if [ $# -gt 0 ] && [ -d "$1" ]; then root=$(cd "$1" && pwd); shift; fi
raw=$(dirname "$out")/_trace_raw
rm -rf "$raw"; mkdir -p "$(dirname "$out")"
cd "$root" || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$raw" -- python3 bench.py --gpus 1 --steps 20 --warmup 5 "$@" > "$out.bench.json" 2> "$out.err"
rc=$?
echo "rocprofv3 exit $rc"
[ $rc -eq 0 ] || { tail -5 "$out.err"; exit $rc; }
python3 "$here/tools/trace_overlap.py" "$raw" "$out" "$(tail -1 "$out.bench.json")"
rm -rf "$raw" "$out.err" "$out.bench.json"
