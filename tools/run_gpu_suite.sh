# One gpurun call: the whole -m gpu suite, then the default bench line (run from the repo root on the GPU box).
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${1:?usage: tools/run_gpu_suite.sh OUTPUT_DIR (relative to the repository root)}
mkdir -p $OUT
timeout -k 10 1000 python -m pytest tests -x -q -m gpu --durations=15 > $OUT/r4_pytest.log 2>&1
rc=$?
echo "pytest rc=$rc"; tail -25 $OUT/r4_pytest.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 400 python3 bench.py --full > $OUT/r4_bench.json 2> $OUT/r4_bench.err
rc=$?
echo "bench rc=$rc"; cut -c1-1500 $OUT/r4_bench.json; tail -3 $OUT/r4_bench.err
exit $rc
