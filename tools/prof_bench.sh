#!/bin/bash
# usage (on an MI355X): bash tools/prof_bench.sh <tag> [bench args...]
# rocprofv3 kernel trace + stats of bench.py --full; writes $OUT/prof_<tag>/ (OUT defaults to out/) and a markdown summary.
TAG=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o p -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline "$@" > $OUT/prof_$TAG.log 2>&1
cd $R
python tools/rocprof_summary.py $OUT/prof_$TAG/p_results.db "bench.py --full --steps 3 --warmup 1 $* (4 passes profiled)" > $OUT/prof_$TAG.md
head -30 $OUT/prof_$TAG.md
