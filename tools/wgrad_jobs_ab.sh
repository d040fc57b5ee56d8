#!/bin/bash
# A/B of the weight-gradient launch against a parent tree, with one per-call switch of this tree as the third arm (default
# PP_WGRAD_JOBROT: the 64-row `outer` job and the rotated job list; PP_WGRAD_WIDE: the 16-byte loop - DESIGN.md 4.1 / 8):
#   bash tools/wgrad_jobs_ab.sh <parent tree> [tag] [output directory] [part: bench | trace | all] [switch] [arm name, default rot]
# <parent tree>: a checkout of the parent commit with its library built. bench: alternating bench.py runs of the parent, this tree and
# this tree with <switch>=0 (headline step, the driver's short command, the ragged workload, --lstm-dim 1024), dumped outputs of
# the last timed step; trace: rocprofv3 kernel traces in runs of their own and the per-workgroup timelines
# (tools/wg_trace_wgrad_single.py; the parent tree gets a copy of the tool).
# Output: <output directory, default profile_out>/<tag>_wgrad_jobs_ab.txt, _wgrad_jobs_dumps.txt, _h1024_ab.txt,
# <tag>_{parent,<arm>1,<arm>0}_train_{kernel_stats,step_sequence,gaps}.csv, <tag>_{parent,<arm>1}_train_gumm_*.csv, <tag>_{parent,<arm>1}_wgrad_wg_trace.txt
set -o pipefail
REPO=$PWD; PAR=$(cd ${1:?parent tree} && pwd); TAG=${2:-wj}; OUT=${3:-$PWD/profile_out}; PART=${4:-all}; SW=${5:-PP_WGRAD_JOBROT}; ARM=${6:-rot}; mkdir -p $OUT; OUT=$(cd $OUT && pwd)
run() {  # file, label, tree, switch, args...
  local ab=$1 label=$2 tree=$3 cs=$4; shift 4
  ( cd $tree && env $SW=$cs timeout -k 10 240 python bench.py --gpus 1 "$@" --no-cpu-baseline 2>$OUT/final_err.txt | tail -1 | python -c "
import sys, json
d = json.loads(sys.stdin.read())
print('$label', '$*', json.dumps({k: d.get(k) for k in ('value', 'ms_per_step')}))" >> $ab ) || exit 1
  tail -1 $ab
}
if [ $PART = bench ] || [ $PART = all ]; then
AB=$OUT/${TAG}_wgrad_jobs_ab.txt; : > $AB
for i in 1 2 3 4 5 6; do run $AB parent $PAR 1 --steps 200 --warmup 20 --no-is && run $AB new $REPO 1 --steps 200 --warmup 20 --no-is && run $AB new_${ARM}0 $REPO 0 --steps 200 --warmup 20 --no-is || exit 1; done
for i in 1 2 3 4 5; do run $AB parent $PAR 1 --steps 20 --warmup 5 --no-is && run $AB new $REPO 1 --steps 20 --warmup 5 --no-is || exit 1; done
for i in 1 2 3 4; do run $AB parent $PAR 1 --workload train_gumm --steps 100 --warmup 10 && run $AB new $REPO 1 --workload train_gumm --steps 100 --warmup 10 || exit 1; done
H=$OUT/${TAG}_h1024_ab.txt; : > $H
for i in 1 2 3 4; do run $H parent $PAR 1 --lstm-dim 1024 --steps 200 --warmup 20 --no-is && run $H new $REPO 1 --lstm-dim 1024 --steps 200 --warmup 20 --no-is || exit 1; done
# dumped outputs: two parent runs against each other, then parent against new
for t in parent_a parent_b; do ( cd $PAR && timeout -k 10 240 python bench.py --gpus 1 --steps 200 --warmup 20 --no-cpu-baseline --no-is --dump-outputs $OUT/dump_$t > /dev/null 2>&1 ) || exit 1; done
( cd $REPO && timeout -k 10 240 python bench.py --gpus 1 --steps 200 --warmup 20 --no-cpu-baseline --no-is --dump-outputs $OUT/dump_new > /dev/null 2>&1 ) || exit 1
python tools/compare_dumps.py $OUT/dump_parent_a $OUT/dump_parent_b parent_vs_parent > $OUT/${TAG}_wgrad_jobs_dumps.txt && python tools/compare_dumps.py $OUT/dump_parent_a $OUT/dump_new parent_vs_new >> $OUT/${TAG}_wgrad_jobs_dumps.txt || exit 1
cat $OUT/${TAG}_wgrad_jobs_dumps.txt; rm -rf $OUT/dump_*
fi
[ $PART = trace ] || [ $PART = all ] || exit 0
# kernel traces, each in its own run (the profiler's program goes after --)
export TMPDIR=/tmp
trace() {  # tag, tree, switch, seq name, extra args
  local tag=$1 tree=$2 cs=$3 seq=$4; shift 4
  rm -rf $OUT/fp_ks
  ( cd $tree && env $SW=$cs timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/fp_ks -o p -- python bench.py --steps 200 --warmup 20 --no-cpu-baseline --no-is "$@" > $OUT/ks_$tag.log 2>&1 ) || exit 1
  python $REPO/tools/rocprof_summary.py $OUT/fp_ks/p_results.db $OUT/${tag}_kernel_stats.csv > /dev/null || exit 1
  python -c "
import sys; sys.path.insert(0, '$REPO/tools')
import rocprof_summary as R
R.sequence('$OUT/fp_ks/p_results.db', '$OUT/${tag}_${seq}.csv')" || exit 1
  python $REPO/tools/kernel_gaps.py $OUT/fp_ks/p_results.db $OUT/${tag}_gaps.csv > /dev/null || exit 1
  rm -rf $OUT/fp_ks $OUT/ks_$tag.log
  echo "== $tag"; cut -c1-120 $OUT/${tag}_gaps.csv | head -8
}
trace ${TAG}_parent_train $PAR 1 step_sequence && trace ${TAG}_${ARM}1_train $REPO 1 step_sequence && trace ${TAG}_${ARM}0_train $REPO 0 step_sequence || exit 1
trace ${TAG}_parent_train_gumm $PAR 1 ragged_step_sequence --workload train_gumm && trace ${TAG}_${ARM}1_train_gumm $REPO 1 ragged_step_sequence --workload train_gumm || exit 1
cp $REPO/tools/wg_trace_wgrad_single.py $PAR/tools/ || exit 1
( cd $PAR && timeout -k 10 120 python tools/wg_trace_wgrad_single.py > $OUT/${TAG}_parent_wgrad_wg_trace.txt 2>&1 ) || exit 1
( cd $REPO && timeout -k 10 120 python tools/wg_trace_wgrad_single.py > $OUT/${TAG}_${ARM}1_wgrad_wg_trace.txt 2>&1 ) || exit 1
