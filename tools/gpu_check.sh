# GPU-box check: gpu tests, smoke, the full bench (graph replay, the default, + eager). Stops at the
# first failure. Logs under $OUT (default: bench_out/ in the repository).
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/t_all.log 2>&1 || { echo "pytest failed rc=$?"; tail -30 $OUT/t_all.log; exit 1; }
tail -3 $OUT/t_all.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { echo "smoke failed"; tail -30 $OUT/smoke.log; exit 1; }
tail -1 $OUT/smoke.log
timeout -k 10 400 python bench.py --full > $OUT/bench.log 2>&1 || { echo "bench failed"; tail -30 $OUT/bench.log; exit 1; }
tail -1 $OUT/bench.log
timeout -k 10 300 python bench.py --full --eager --no-cpu-baseline --no-all-slots-rate > $OUT/bench_eager.log 2>&1 || { echo "bench eager failed"; tail -30 $OUT/bench_eager.log; exit 1; }
tail -1 $OUT/bench_eager.log
