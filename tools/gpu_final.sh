# End-of-round evidence on one MI355X: the GPU suite, the full default bench
# line, then tools/profile.sh (kernel trace + PMC passes) of the same workload.
# Usage, from the repository root: bash tools/gpu_final.sh TAG
# (OUT: the directory the logs, the bench line and profile.sh's prof_TAG go to, default bench_out)
set -o pipefail
TAG=${1:-r04}
export OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 250 --timeout-method thread > $OUT/final_tests.log 2>&1 || { echo TESTFAIL; grep -E "^FAILED|^E " $OUT/final_tests.log | head -20; exit 1; }
tail -1 $OUT/final_tests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/final_smoke.log 2>&1 || { echo SMOKEFAIL; tail -5 $OUT/final_smoke.log; exit 1; }
tail -1 $OUT/final_smoke.log
timeout -k 10 400 python bench.py --full > $OUT/final_bench.json 2> $OUT/final_bench.err || { echo BENCHFAIL; tail -5 $OUT/final_bench.err; exit 1; }
python -c "import json;d=json.load(open('$OUT/final_bench.json'));print(round(d['value'],1),d['ms_per_step'],d['roofline'],d['cpu_baseline']['value'])"
bash tools/profile.sh $TAG
