#!/bin/bash
# Bench lines of the other configs on one GPU (no CPU baseline): C1, C2, museum, C5, C4.
# (OUT: the directory the logs and bench lines go to, default bench_out)
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
for c in ${@:-c1 c2 museum c5 c4}; do
  steps=3; [ $c == c4 ] && steps=1; [ $c == c1 ] && steps=20
  timeout -k 10 300 python bench.py --config $c --steps $steps --warmup 1 > $OUT/cfg_$c.json 2> $OUT/cfg_$c.err || { echo FAIL $c; tail -5 $OUT/cfg_$c.err; exit 1; }
  python -c "import json;d=json.loads(open('$OUT/cfg_$c.json').read().strip().splitlines()[-1]);print('$c', round(d['value']), 'Mray/s', round(d['ms_per_step'],2), 'ms/step', d['kernel_busy_ms_per_step'])"
done
