# Data-parallel / graph-replay checks on one box (gloo world 2 on the one GPU, RCCL world 1), then
# the full bench line. Usage: TAG=... [OUT=<dir>] bash tools/dp_check.sh   (logs under $OUT, default bench_out/)
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT
TAG=${TAG:-r6dp}
timeout -k 10 900 python -u -m pytest -x -v --timeout 300 --timeout-method thread -p no:cacheprovider \
    tests/test_graph_dp_gpu.py tests/test_nccl_gpu.py tests/test_dp_gpu.py tests/test_graph_gpu.py \
    tests/test_bench_gpu.py > $OUT/${TAG}_dp_tests.log 2>&1 || { echo "pytest failed rc=$?"; tail -40 $OUT/${TAG}_dp_tests.log; exit 1; }
tail -3 $OUT/${TAG}_dp_tests.log
timeout -k 10 600 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { echo "bench failed"; tail -30 $OUT/${TAG}_bench.err; exit 1; }
python -c "import json; d=json.load(open('$OUT/${TAG}_bench.json')); print(d['value'], d['ms_per_step'], d.get('all_slots_iters_s'), d.get('k16_iters_s'), d.get('side_rates_mode'), d['roofline']['frac'])"
