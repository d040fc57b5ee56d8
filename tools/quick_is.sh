# the GUM posterior call through the API: bench record with and without pp_is_first_statement   (bash tools/quick_is.sh <tag>)
REPO=$PWD; mkdir -p "${OUT:?set OUT to the directory for the result files}"; OUT=$(cd "$OUT" && pwd)
TAG=${1:-q}
for f in 1 0; do
PP_IS_FIRST=$f python bench.py --workload is --full --no-cpu-baseline > $OUT/${TAG}_is_first$f.json 2> $OUT/${TAG}_is_first$f.err
tail -2 $OUT/${TAG}_is_first$f.err | cut -c1-300
python -c "
import json
d=json.loads(open('$OUT/${TAG}_is_first$f.json').read().strip().splitlines()[-1])
r=d.get('is', d)
print('PP_IS_FIRST=$f', d.get('value'), {k: r.get(k) for k in ('particles_per_sec','ms_per_call','plan_replays','noplan','device_chain')})
"
done
