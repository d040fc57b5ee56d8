#!/bin/bash
# A/B of the first launch's early order (PP_FIRST_EARLY) against a parent tree, the switch-off arm third:
#   bash tools/first_launch_ab.sh <parent tree> [tag] [output directory] [parts, comma separated; default all]
# <parent tree>: a checkout of the parent commit with its library built. Parts (each appends to / writes its own files, so a
# long A/B can be split over several invocations):
#   headline  six rounds of parent / new / new with PP_FIRST_EARLY=0: bench.py --steps 200 --warmup 20 --no-is
#   short     five rounds of the driver's short command (--steps 20 --warmup 5 --no-is), the same three arms
#   gumm      four rounds of --workload train_gumm --steps 100 --warmup 10, parent / new
#   h1024     four rounds of --lstm-dim 1024 --steps 200 --warmup 20 --no-is, parent / new
#   dumps     --dump-outputs: two parent runs against each other, then parent against new (tools/compare_dumps.py)
#   trace     rocprofv3 --kernel-trace --stats of the headline step, one run per arm, with tools/kernel_gaps.py; the ragged step
#             (--workload train_gumm) for parent and new
#   wgtrace   tools/first_launch_wg_trace.py on this tree with the switch at 0 (the parent's order with stamps) and at 1
# (The IS first-statement kernel keeps the staging it had: no `is` part.)
# Output: <output directory, default profile_out>/<tag>_first_launch_ab.txt, _h1024_ab.txt, _first_launch_dumps.txt,
# <tag>_{parent,early1,early0}_train_{kernel_stats,step_sequence,gaps}.csv, <tag>_{parent,early1}_train_gumm_kernel_stats.csv,
# <tag>_{parent,early1}_first_wg_trace.txt
set -o pipefail
REPO=$PWD; PAR=$(cd ${1:?parent tree} && pwd); TAG=${2:-fe}; OUT=${3:-$PWD/profile_out}; PARTS=${4:-all}; mkdir -p $OUT; OUT=$(cd $OUT && pwd)
SW=PP_FIRST_EARLY
has() { [ $PARTS = all ] || [[ ",$PARTS," == *",$1,"* ]]; }
run() {  # file, label, tree, switch value, args...
  local ab=$1 label=$2 tree=$3 cs=$4; shift 4
  ( cd $tree && env $SW=$cs timeout -k 10 240 python bench.py --gpus 1 "$@" --no-cpu-baseline 2>$OUT/final_err.txt | tail -1 | python -c "
import sys, json
d = json.loads(sys.stdin.read())
print('$label', '$*', json.dumps({k: d.get(k) for k in ('value', 'ms_per_step')}))" >> $ab ) || exit 1
  tail -1 $ab
}
AB=$OUT/${TAG}_first_launch_ab.txt
if has headline; then
for i in 1 2 3 4 5 6; do run $AB parent $PAR 1 --steps 200 --warmup 20 --no-is && run $AB new $REPO 1 --steps 200 --warmup 20 --no-is && run $AB new_early0 $REPO 0 --steps 200 --warmup 20 --no-is || exit 1; done
fi
if has short; then
for i in 1 2 3 4 5; do run $AB parent $PAR 1 --steps 20 --warmup 5 --no-is && run $AB new $REPO 1 --steps 20 --warmup 5 --no-is && run $AB new_early0 $REPO 0 --steps 20 --warmup 5 --no-is || exit 1; done
fi
if has gumm; then
for i in 1 2 3 4; do run $AB parent $PAR 1 --workload train_gumm --steps 100 --warmup 10 && run $AB new $REPO 1 --workload train_gumm --steps 100 --warmup 10 || exit 1; done
fi
if has h1024; then
H=$OUT/${TAG}_h1024_ab.txt
for i in 1 2 3 4; do run $H parent $PAR 1 --lstm-dim 1024 --steps 200 --warmup 20 --no-is && run $H new $REPO 1 --lstm-dim 1024 --steps 200 --warmup 20 --no-is || exit 1; done
fi
if has dumps; then
# dumped outputs: two parent runs against each other, then parent against new
for t in parent_a parent_b; do ( cd $PAR && timeout -k 10 240 python bench.py --gpus 1 --steps 200 --warmup 20 --no-cpu-baseline --no-is --dump-outputs $OUT/dump_$t > /dev/null 2>&1 ) || exit 1; done
( cd $REPO && timeout -k 10 240 python bench.py --gpus 1 --steps 200 --warmup 20 --no-cpu-baseline --no-is --dump-outputs $OUT/dump_new > /dev/null 2>&1 ) || exit 1
python tools/compare_dumps.py $OUT/dump_parent_a $OUT/dump_parent_b parent_vs_parent > $OUT/${TAG}_first_launch_dumps.txt && python tools/compare_dumps.py $OUT/dump_parent_a $OUT/dump_new parent_vs_new >> $OUT/${TAG}_first_launch_dumps.txt || exit 1
cat $OUT/${TAG}_first_launch_dumps.txt; rm -rf $OUT/dump_*
fi
if has trace; then
# kernel traces, each in its own run (the profiler's program goes after --)
export TMPDIR=/tmp
trace() {  # tag, tree, switch value, full (1: step sequence and gaps too), bench arguments...
  local tag=$1 tree=$2 cs=$3 full=$4; shift 4
  rm -rf $OUT/fp_ks
  ( cd $tree && env $SW=$cs timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/fp_ks -o p -- python bench.py "$@" --no-cpu-baseline > $OUT/ks_$tag.log 2>&1 ) || exit 1
  python $REPO/tools/rocprof_summary.py $OUT/fp_ks/p_results.db $OUT/${tag}_kernel_stats.csv > /dev/null || exit 1
  if [ $full = 1 ]; then
  python -c "
import sys; sys.path.insert(0, '$REPO/tools')
import rocprof_summary as R
R.sequence('$OUT/fp_ks/p_results.db', '$OUT/${tag}_step_sequence.csv')" || exit 1
  python $REPO/tools/kernel_gaps.py $OUT/fp_ks/p_results.db $OUT/${tag}_gaps.csv > /dev/null || exit 1
  echo "== $tag"; cut -c1-120 $OUT/${tag}_gaps.csv | head -8
  fi
  rm -rf $OUT/fp_ks $OUT/ks_$tag.log
}
HL="--steps 200 --warmup 20 --no-is"
trace ${TAG}_parent_train $PAR 1 1 $HL && trace ${TAG}_early1_train $REPO 1 1 $HL && trace ${TAG}_early0_train $REPO 0 1 $HL || exit 1
GM="--workload train_gumm --steps 100 --warmup 10"
trace ${TAG}_parent_train_gumm $PAR 1 0 $GM && trace ${TAG}_early1_train_gumm $REPO 1 0 $GM || exit 1
fi
if has wgtrace; then
( cd $REPO && PP_FIRST_EARLY=0 timeout -k 10 120 python tools/first_launch_wg_trace.py > $OUT/${TAG}_parent_first_wg_trace.txt 2>&1 ) || exit 1
( cd $REPO && PP_FIRST_EARLY=1 timeout -k 10 120 python tools/first_launch_wg_trace.py > $OUT/${TAG}_early1_first_wg_trace.txt 2>&1 ) || exit 1
fi
