# bench.py's kernel-bound event timing against rocprofv3 --kernel-trace of the same command
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}
mkdir -p $OUT
cd $R
python bench.py --full --steps 100 --warmup 5 --no-cpu-baseline > $OUT/agree_bench.json 2> $OUT/agree.err
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $OUT/prof_agree -o pipe -- python3 $R/bench.py --full --steps 20 --warmup 3 --isolated 0 --no-cpu-baseline > $OUT/agree_prof_bench.json 2>> $OUT/agree.err
cd $R
DB=$(find $OUT/prof_agree -name "pipe_results.db" | head -1)
python tools/rocprof_summary.py "$DB" "bench.py (pipelined)" > $OUT/agree_prof.md 2>&1
rm -rf $OUT/prof_agree
