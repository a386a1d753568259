# Full check on one box: the whole GPU suite once (-x, multi-process rehearsals last), smoke,
# the full bench line (bench.py --full), then (AB=<lib.so>) a whole-step A/B of the in-tree library
# against that build. Logs under $OUT (default: bench_out/ in the repository).
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT
TAG=${TAG:-r6a}
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -q --timeout 400 --timeout-method thread -p no:cacheprovider > $OUT/${TAG}_gpu_tests.log 2>&1 || { echo "pytest failed rc=$?"; tail -40 $OUT/${TAG}_gpu_tests.log; exit 1; }
tail -3 $OUT/${TAG}_gpu_tests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1 || { echo "smoke failed"; tail -30 $OUT/${TAG}_smoke.log; exit 1; }
tail -2 $OUT/${TAG}_smoke.log
timeout -k 10 400 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { echo "bench failed"; tail -30 $OUT/${TAG}_bench.err; exit 1; }
python -c "import json; d=json.load(open('$OUT/${TAG}_bench.json')); print(d['value'], d['ms_per_step'], d['roofline'])"
if [ -n "$AB" ]; then bash tools/gpu_lib_ab.sh $AB 3 > $OUT/${TAG}_step_ab.log 2>&1 || { tail -20 $OUT/${TAG}_step_ab.log; exit 1; }; cat $OUT/${TAG}_step_ab.log; fi
