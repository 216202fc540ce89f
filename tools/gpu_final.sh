# Round-end style check on one MI355X: full GPU tests, smoke, headline bench, per-kernel stats.
#   bash tools/gpu_final.sh <tag>          (results under $OUT_DIR, default bench_out)
set -o pipefail
tag=${1:-final}
out=${OUT_DIR:-bench_out}
mkdir -p $out
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread \
    > $out/pytest_$tag.log 2>&1 && \
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > $out/smoke_$tag.log 2>&1 && \
timeout -k 10 300 python bench.py --full > $out/bench_default_$tag.json 2> $out/bench_default_$tag.err && \
timeout -k 10 300 python bench.py --steps 50 --warmup 10 --full > $out/bench_$tag.json 2> $out/bench_$tag.err && \
timeout -k 10 300 python bench.py --model lenet --steps 200 --warmup 20 --full > $out/bench_lenet_$tag.json 2> $out/bench_lenet_$tag.err && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_$tag -o prof -- \
    python bench.py --steps 7 --warmup 3 > $out/prof_$tag.log 2>&1
rc=$?
tail -3 $out/pytest_$tag.log; tail -1 $out/smoke_$tag.log; cat $out/bench_default_$tag.json $out/bench_$tag.json $out/bench_lenet_$tag.json
exit $rc
