#!/bin/bash
# A/B of the forward embedding in the panel kernel's staging phase (PP_PANEL_EMBED) against a parent tree,
# the switch-off arm third (the sibling of tools/first_launch_ab.sh):
#   bash tools/panel_embed_ab.sh <parent tree> [tag] [output directory] [parts, comma separated; default all]
# <parent tree>: a checkout of the parent commit with its library built. Parts (each appends to / writes its own files, so a
# long A/B can be split over several invocations):
#   headline  six rounds of parent / new / new with PP_PANEL_EMBED=0: bench.py --steps 200 --warmup 20 --no-is
#   short     five rounds of the driver's short command (--steps 20 --warmup 5 --no-is), the same three arms
#   gumm      four rounds of --workload train_gumm --steps 100 --warmup 10, parent / new (the ragged step: its path is unchanged)
#   h1024     four rounds of --lstm-dim 1024 --steps 200 --warmup 20 --no-is, parent / new
#   dumps     --dump-outputs: two parent runs against each other, then parent against new (tools/compare_dumps.py)
#   trace     rocprofv3 --kernel-trace --stats of the headline step at --steps 5000 (5 000 launches of each kernel per
#             recording), two recordings per arm, arms alternating
#   timeline  tools/panel_timeline.py (phase stamps of the panel kernel) and tools/first_launch_wg_trace.py (workgroups of the
#             first launch) on this tree with the switch at 0 (the parent's order with stamps) and at 1
# Output: <output directory, default profile_out>/<tag>_ab.txt, <tag>_h1024_ab.txt, <tag>_dumps.txt,
# <tag>_{parent,embed1,embed0}_{a,b}_train_kernel_stats.csv, <tag>_{embed0,embed1}_panel16_timeline.txt, _first_wg_trace.txt
set -o pipefail
REPO=$PWD; PAR=$(cd ${1:?parent tree} && pwd); TAG=${2:-pe}; OUT=${3:-$PWD/profile_out}; PARTS=${4:-all}; mkdir -p $OUT; OUT=$(cd $OUT && pwd)
SW=PP_PANEL_EMBED
has() { [ $PARTS = all ] || [[ ",$PARTS," == *",$1,"* ]]; }
run() {  # file, label, tree, switch value, args...
  local ab=$1 label=$2 tree=$3 cs=$4; shift 4
  ( cd $tree && env $SW=$cs timeout -k 10 240 python bench.py --gpus 1 "$@" --no-cpu-baseline 2>$OUT/final_err.txt | tail -1 | python -c "
import sys, json
d = json.loads(sys.stdin.read())
print('$label', '$*', json.dumps({k: d.get(k) for k in ('value', 'ms_per_step')}))" >> $ab ) || exit 1
  tail -1 $ab
}
AB=$OUT/${TAG}_ab.txt
if has headline; then
for i in 1 2 3 4 5 6; do run $AB parent $PAR 1 --steps 200 --warmup 20 --no-is && run $AB new $REPO 1 --steps 200 --warmup 20 --no-is && run $AB new_embed0 $REPO 0 --steps 200 --warmup 20 --no-is || exit 1; done
fi
if has short; then
for i in 1 2 3 4 5; do run $AB parent $PAR 1 --steps 20 --warmup 5 --no-is && run $AB new $REPO 1 --steps 20 --warmup 5 --no-is && run $AB new_embed0 $REPO 0 --steps 20 --warmup 5 --no-is || exit 1; done
fi
if has gumm; then
for i in 1 2 3 4; do run $AB parent $PAR 1 --workload train_gumm --steps 100 --warmup 10 && run $AB new $REPO 1 --workload train_gumm --steps 100 --warmup 10 || exit 1; done
fi
if has h1024; then
H=$OUT/${TAG}_h1024_ab.txt
for i in 1 2 3 4; do run $H parent $PAR 1 --lstm-dim 1024 --steps 200 --warmup 20 --no-is && run $H new $REPO 1 --lstm-dim 1024 --steps 200 --warmup 20 --no-is || exit 1; done
fi
if has dumps; then
for t in parent_a parent_b; do ( cd $PAR && timeout -k 10 240 python bench.py --gpus 1 --steps 200 --warmup 20 --no-cpu-baseline --no-is --dump-outputs $OUT/dump_$t > /dev/null 2>&1 ) || exit 1; done
( cd $REPO && timeout -k 10 240 python bench.py --gpus 1 --steps 200 --warmup 20 --no-cpu-baseline --no-is --dump-outputs $OUT/dump_new > /dev/null 2>&1 ) || exit 1
python tools/compare_dumps.py $OUT/dump_parent_a $OUT/dump_parent_b parent_vs_parent > $OUT/${TAG}_dumps.txt && python tools/compare_dumps.py $OUT/dump_parent_a $OUT/dump_new parent_vs_new >> $OUT/${TAG}_dumps.txt || exit 1
cat $OUT/${TAG}_dumps.txt; rm -rf $OUT/dump_*
fi
if has trace; then
# kernel traces, each in its own run (the profiler's program goes after --)
export TMPDIR=/tmp
trace() {  # tag, tree, switch value
  local tag=$1 tree=$2 cs=$3
  rm -rf $OUT/fp_ks
  ( cd $tree && env $SW=$cs timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/fp_ks -o p -- python bench.py --steps 5000 --warmup 20 --no-is --no-cpu-baseline > $OUT/ks_$tag.log 2>&1 ) || exit 1
  python $REPO/tools/rocprof_summary.py $OUT/fp_ks/p_results.db $OUT/${tag}_train_kernel_stats.csv > /dev/null || exit 1
  echo "== $tag"; grep -E 'panel16|wgrad_t1|obs_embed_fwd|live_adam' $OUT/${tag}_train_kernel_stats.csv | cut -c1-160
  rm -rf $OUT/fp_ks $OUT/ks_$tag.log
}
for r in a b; do trace ${TAG}_parent_$r $PAR 1 && trace ${TAG}_embed1_$r $REPO 1 && trace ${TAG}_embed0_$r $REPO 0 || exit 1; done
fi
if has timeline; then
for cs in 0 1; do
( cd $REPO && env $SW=$cs timeout -k 10 120 python tools/panel_timeline.py > $OUT/${TAG}_embed${cs}_panel16_timeline.txt 2>&1 ) || exit 1
( cd $REPO && env $SW=$cs timeout -k 10 120 python tools/first_launch_wg_trace.py > $OUT/${TAG}_embed${cs}_first_wg_trace.txt 2>&1 ) || exit 1
done
fi
