REPO=$PWD; mkdir -p "${OUT:?set OUT to the directory for the result files}"; OUT=$(cd "$OUT" && pwd)
python bench.py --steps 20 --warmup 5 --full --no-is --no-cpu-baseline > $OUT/r05c_bench.json 2> $OUT/r05c_bench.err
python -c "
import json
d=json.loads(open('$OUT/r05c_bench.json').read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d['roofline']['kernel'][:20], d['roofline']['avg_launch_us'])
"
python tools/panel_timeline.py 2>&1 | tail -4 > $OUT/r05c_panel16_timeline.txt; cat $OUT/r05c_panel16_timeline.txt
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $OUT/fp_ks -o p -- python $REPO/bench.py --steps 200 --warmup 20 --full --no-cpu-baseline --no-is > /dev/null 2>&1
cd $REPO
python tools/rocprof_summary.py $OUT/fp_ks/p_results.db $OUT/r05c_train_kernel_stats.csv > /dev/null
python -c "
import sys; sys.path.insert(0,'tools')
import rocprof_summary as R
R.sequence('$OUT/fp_ks/p_results.db', '$OUT/r05c_step_sequence.csv')
"
rm -rf $OUT/fp_ks
head -8 $OUT/r05c_train_kernel_stats.csv | cut -c1-200
