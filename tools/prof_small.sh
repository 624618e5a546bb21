#!/bin/bash
# Kernel traces of the small-batch workloads: C5 (one step) and the init-default session.
export TMPDIR=/tmp
# (OUT: the directory the logs and bench lines go to, default bench_out)
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_c5 -o run --output-format csv -- python3 bench.py --config c5 --full --steps 1 --warmup 0 --no-cpu-baseline --no-serial-step > $OUT/prof_c5.log 2>&1 || { echo C5FAIL; tail -5 $OUT/prof_c5.log; exit 1; }
python3 tools/timeline.py $OUT/prof_c5 > $OUT/timeline_c5.json && head -12 $OUT/timeline_c5.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_ds -o run --output-format csv -- python3 tools/default_session_rate.py 3 > $OUT/prof_ds.log 2>&1 || { echo DSFAIL; tail -5 $OUT/prof_ds.log; exit 1; }
python3 tools/timeline.py $OUT/prof_ds > $OUT/timeline_ds.json && head -12 $OUT/timeline_ds.json
echo prof-done
