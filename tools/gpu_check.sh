#!/bin/bash
# GPU check used during development: parity suite, then C3 bench lines for the
# given library variants ("" = the product build). Usage: tools/gpu_check.sh [variant ...]
# (OUT: the directory the logs and bench lines go to, default bench_out)
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/t.log 2>&1 || { echo TESTFAIL; tail -30 $OUT/t.log; exit 1; }
tail -1 $OUT/t.log
for v in "" "$@"; do
  WPT_LIB_VARIANT=$v timeout -k 10 200 python bench.py --full --no-cpu-baseline --steps 5 > $OUT/b_$v.json 2>$OUT/b_$v.err || { echo BENCHFAIL $v; tail $OUT/b_$v.err; exit 1; }
  python -c "import json;d=json.load(open('$OUT/b_$v.json'));print('[$v]',round(d['value']),round(d['ms_per_step'],2),d['kernel_busy_ms_per_step'],d['work'])"
done
timeout -k 10 200 python bench.py --steps 3 --opt lanes=1 > $OUT/b_l1.json 2>$OUT/b_l1.err && python -c "import json;d=json.load(open('$OUT/b_l1.json'));print('lanes1',round(d['value']),d['ms_per_step'],d['kernel_launch_ms_per_step'])"
