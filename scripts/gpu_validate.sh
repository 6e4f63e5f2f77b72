set -x
# usage: bash scripts/gpu_validate.sh <output directory>
R=$PWD
OUT=$(mkdir -p "${1:?usage: gpu_validate.sh <output directory>}" && cd "$1" && pwd)
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
timeout 1500 python -m pytest tests -m gpu -x -q 2>&1 | tail -2
# the driver's command with everything the line can carry (--full): one JSON line
timeout 900 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err; tail -1 $OUT/bench_default.json | cut -c1-1800
# same command under rocprofv3 (kernel trace + stats): steady-state step breakdown + the roofline kernel's average
# (no live counter passes under the trace)
mkdir -p $OUT/prof_default; cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -f csv -d $OUT/prof_default/trace -o t -- python $R/bench.py --steps 8 --warmup 4 --full --no-live-traffic --no-cpu-baseline --no-secondary > $OUT/prof_default/trace.log 2>&1
cd $R
f=$(find $OUT/prof_default/trace -name '*kernel_trace.csv' | head -1)
python scripts/steady_state.py $f assign_anchor_kernel 4 5 > $OUT/prof_default/steady_state.txt
head -3 $OUT/prof_default/steady_state.txt | cut -c1-200
k=$(find $OUT/prof_default/trace -name '*kernel_stats.csv' | head -1)
head -1 $k > $OUT/prof_default/roofline_kernel_stats.csv
grep "roi_align_fwd_merged_kernel\|roi_order_kernel" $k >> $OUT/prof_default/roofline_kernel_stats.csv
cat $OUT/prof_default/roofline_kernel_stats.csv | cut -c1-300
rm -rf $OUT/prof_default/trace
