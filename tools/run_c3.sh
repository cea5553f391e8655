# configs[3] at its per-GPU size (the full-size test), then the default bench line without the CPU baseline
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${1:?usage: tools/run_c3.sh OUTPUT_DIR (relative to the repository root)}
mkdir -p $OUT
timeout -k 10 500 python -m pytest tests/test_gpu_selfplay.py -x -q -k "configs3" > $OUT/r3_c3_pytest.log 2>&1
rc=$?
echo "pytest rc=$rc"; grep -a "hivemind_amd error" $OUT/r3_c3_pytest.log | cut -c1-3000 | tail -2; tail -3 $OUT/r3_c3_pytest.log
[ $rc -eq 124 ] && exit 124
[ $rc -eq 137 ] && exit 137
timeout -k 10 400 python3 bench.py --full --no-cpu-baseline > $OUT/r3_bench.json 2> $OUT/r3_bench.err
rc2=$?
echo "bench rc=$rc2"; cut -c1-1200 $OUT/r3_bench.json; tail -3 $OUT/r3_bench.err
exit $rc
