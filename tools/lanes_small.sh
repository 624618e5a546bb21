#!/bin/bash
# Same-session A/B on the small-batch workloads (C5 adaptive rounds and the
# init-default session). Each argument is NAME=ENV (space-separated
# assignments, e.g. "sl2=WPT_SMALL_LANES=2"); "base=" runs the product as is.
# (OUT: the directory the logs and bench lines go to, default bench_out)
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
for spec in "$@"; do
  name=${spec%%=*}; envs=${spec#*=}
  env $envs timeout -k 10 300 python bench.py --config c5 --steps 2 --warmup 1 > $OUT/c5_$name.json 2> $OUT/c5_$name.err || { echo FAIL c5 $name; tail -5 $OUT/c5_$name.err; exit 1; }
  python -c "import json;d=json.loads(open('$OUT/c5_$name.json').read().strip().splitlines()[-1]);print('c5 $name', round(d['value']), 'Mray/s', round(d['ms_per_step'],1), 'ms/step')"
  env $envs timeout -k 10 300 python tools/default_session_rate.py 4 > $OUT/ds_$name.json 2> $OUT/ds_$name.err || { echo FAIL ds $name; tail -5 $OUT/ds_$name.err; exit 1; }
  python -c "import json;d=json.load(open('$OUT/ds_$name.json'));print('init-defaults $name', round(d['Mray/s']), 'Mray/s')"
done
