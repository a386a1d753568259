# GPU-box profile of the headline step (bench.py config 2 without the side measurements):
#   1. rocprofv3 --kernel-trace --stats           -> <tag>_stats/ (stats CSV) + the bench line under it
#   2. rocprofv3 --kernel-trace (no --stats)      -> per-kernel stats computed by tools/trace_stats.py
# The bench's own roofline.avg_launch_ms (HIP events; bench.py --full) is printed by both runs for comparison.
# Usage: [OUT=<dir>] bash tools/prof_step.sh <tag> [steps]   (outputs under $OUT, default bench_out/ in the repository)
set -o pipefail
T=${1:-r2}
K=${2:-20}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
B="--full --no-cpu-baseline --no-all-slots-rate --no-k16-rate --no-breakdown --no-extras --steps $K"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/${T}_stats -o step --output-format csv -- python3 $R/bench.py $B > $OUT/${T}_stats.log 2>&1 || { echo "stats run failed rc=$?"; tail -20 $OUT/${T}_stats.log; exit 1; }
tail -1 $OUT/${T}_stats.log
timeout -k 10 300 rocprofv3 --kernel-trace -d $OUT/${T}_trace -o step --output-format csv -- python3 $R/bench.py $B > $OUT/${T}_trace.log 2>&1 || { echo "trace run failed rc=$?"; tail -20 $OUT/${T}_trace.log; exit 1; }
tail -1 $OUT/${T}_trace.log
cd $R
# all launches, and only the timed steps (bench default, graph replay: 1 GEMM-timer eager step + 4 warmup steps (eager + capture) + K replayed steps)
python3 tools/trace_stats.py $OUT/${T}_trace $OUT/${T}_trace_stats.csv --top 60 > $OUT/${T}_trace_top.txt
python3 tools/trace_stats.py $OUT/${T}_trace $OUT/${T}_trace_timed_stats.csv --tail $K/$((K + 5)) --top 60 > $OUT/${T}_trace_timed_top.txt
python3 tools/trace_stats.py $OUT/${T}_stats $OUT/${T}_stats_timed_stats.csv --tail $K/$((K + 5)) --top 5 > /dev/null
# one replayed step's kernel sequence (durations, gaps) for the tail breakdown
python3 tools/trace_seq.py $OUT/${T}_trace > $OUT/${T}_seq.txt 2>&1 || true
find $OUT/${T}_stats $OUT/${T}_trace -name "*kernel_trace.csv" -delete
head -30 $OUT/${T}_trace_top.txt
