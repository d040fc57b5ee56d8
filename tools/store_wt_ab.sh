#!/bin/bash
# A/B of the write-through result stores (PP_STORE_WT): bash tools/store_wt_ab.sh <parent tree> [tag] [output directory]
# <parent tree>: a checkout of the parent commit with its library built. Alternating bench.py runs of the parent, this tree and this
# tree with PP_STORE_WT=0 (headline step, the driver's short command, the ragged workload), dumped outputs of the last timed step,
# then rocprofv3 kernel traces in runs of their own: <output directory, default profile_out>/<tag>_store_wt_ab.txt, _store_wt_dumps.txt,
# <tag>_{parent,wt1,wt0}_train_{kernel_stats,step_sequence,gaps}.csv, <tag>_{parent,wt1}_train_gumm_*.csv
set -o pipefail
REPO=$PWD; PAR=$(cd ${1:?parent tree} && pwd); TAG=${2:-wt}; OUT=${3:-$PWD/profile_out}; mkdir -p $OUT; OUT=$(cd $OUT && pwd)
AB=$OUT/${TAG}_store_wt_ab.txt; : > $AB
run() {  # label, tree, extra env, args...
  local label=$1 tree=$2 wt=$3; shift 3
  ( cd $tree && PP_STORE_WT=$wt timeout -k 10 240 python bench.py --gpus 1 "$@" --no-cpu-baseline 2>$OUT/final_err.txt | tail -1 | python -c "
import sys, json
d = json.loads(sys.stdin.read())
print('$label', '$*', json.dumps({k: d.get(k) for k in ('value', 'ms_per_step')}))" >> $AB ) || exit 1
  tail -1 $AB
}
for i in 1 2 3 4 5 6; do run parent $PAR 1 --steps 200 --warmup 20 && run new $REPO 1 --steps 200 --warmup 20 && run new_wt0 $REPO 0 --steps 200 --warmup 20 || exit 1; done
for i in 1 2 3 4 5; do run parent $PAR 1 --steps 20 --warmup 5 && run new $REPO 1 --steps 20 --warmup 5 || exit 1; done
for i in 1 2 3 4; do run parent $PAR 1 --workload train_gumm --steps 100 --warmup 10 && run new $REPO 1 --workload train_gumm --steps 100 --warmup 10 && run new_wt0 $REPO 0 --workload train_gumm --steps 100 --warmup 10 || exit 1; done
# dumped outputs: two parent runs against each other, then parent against new
for t in parent_a parent_b; do ( cd $PAR && timeout -k 10 240 python bench.py --gpus 1 --steps 200 --warmup 20 --no-cpu-baseline --no-is --dump-outputs $OUT/dump_$t > /dev/null 2>&1 ) || exit 1; done
( cd $REPO && timeout -k 10 240 python bench.py --gpus 1 --steps 200 --warmup 20 --no-cpu-baseline --no-is --dump-outputs $OUT/dump_new > /dev/null 2>&1 ) || exit 1
python tools/compare_dumps.py $OUT/dump_parent_a $OUT/dump_parent_b parent_vs_parent > $OUT/${TAG}_store_wt_dumps.txt && python tools/compare_dumps.py $OUT/dump_parent_a $OUT/dump_new parent_vs_new >> $OUT/${TAG}_store_wt_dumps.txt || exit 1
cat $OUT/${TAG}_store_wt_dumps.txt; rm -rf $OUT/dump_*
# kernel traces, each in its own run
export TMPDIR=/tmp
trace() {  # tag, tree, wt, seq name, extra args
  local tag=$1 tree=$2 wt=$3 seq=$4; shift 4
  rm -rf $OUT/fp_ks
  ( cd $tree && PP_STORE_WT=$wt timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/fp_ks -o p -- python bench.py --steps 200 --warmup 20 --no-cpu-baseline --no-is "$@" > $OUT/ks_$tag.log 2>&1 ) || exit 1
  python $REPO/tools/rocprof_summary.py $OUT/fp_ks/p_results.db $OUT/${tag}_kernel_stats.csv > /dev/null || exit 1
  python -c "
import sys; sys.path.insert(0, '$REPO/tools')
import rocprof_summary as R
R.sequence('$OUT/fp_ks/p_results.db', '$OUT/${tag}_${seq}.csv')" || exit 1
  python $REPO/tools/kernel_gaps.py $OUT/fp_ks/p_results.db $OUT/${tag}_gaps.csv > /dev/null || exit 1
  rm -rf $OUT/fp_ks
  echo "== $tag"; cut -c1-120 $OUT/${tag}_gaps.csv | head -8; cut -c1-100 $OUT/${tag}_${seq}.csv | head -30; head -6 $OUT/${tag}_kernel_stats.csv | cut -c1-60,150-260
}
trace ${TAG}_parent_train $PAR 1 step_sequence && trace ${TAG}_wt1_train $REPO 1 step_sequence && trace ${TAG}_wt0_train $REPO 0 step_sequence || exit 1
trace ${TAG}_parent_train_gumm $PAR 1 ragged_step_sequence --workload train_gumm && trace ${TAG}_wt1_train_gumm $REPO 1 ragged_step_sequence --workload train_gumm || exit 1
