# Standard GPU-box check: GPU test suite, headline bench, per-kernel rocprof stats.
#   bash tools/gpu_run.sh <tag>            (results under $OUT_DIR, default bench_out)
set -o pipefail
tag=${1:-run}
out=${OUT_DIR:-bench_out}
mkdir -p $out
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread \
    > $out/pytest_$tag.log 2>&1 && \
timeout -k 10 300 python bench.py --steps 30 --warmup 5 --full > $out/bench_$tag.json 2> $out/bench_$tag.err && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_$tag -o prof -- \
    python bench.py --steps 7 --warmup 3 --graph 0 > $out/prof_$tag.log 2>&1
rc=$?
tail -3 $out/pytest_$tag.log; cat $out/bench_$tag.json
exit $rc
