# GPU-box profile of the default bench: rocprofv3 kernel-trace stats, then separate FETCH_SIZE and
# WRITE_SIZE PMC passes (MI355X_MICROARCH.md: one TCC counter group per pass), then the per-kernel
# HBM-traffic summary. Usage: [OUT=<dir>] bash tools/gpu_prof.sh <tag>   (outputs under $OUT/<tag>_*,
# OUT defaults to bench_out/ in the repository)
set -o pipefail
T=${1:-r1}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}
mkdir -p $OUT
# --full: pmc_summary.py reads the bench line's roofline object (HIP-event timing of the dominant kernel)
B="--full --no-cpu-baseline --no-all-slots-rate --no-k16-rate --no-breakdown --no-extras"
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/${T}_prof -o step --output-format csv -- python3 $R/bench.py $B --steps 20 > $OUT/${T}_prof.log 2>&1 || { echo "prof failed rc=$?"; tail -20 $OUT/${T}_prof.log; exit 1; }
tail -1 $OUT/${T}_prof.log
timeout -s KILL 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/${T}_pmc_fetch -o pmc --output-format csv -- python3 $R/bench.py $B --steps 2 --warmup 1 > $OUT/${T}_pmc_fetch.log 2>&1 || { echo "fetch pass failed rc=$?"; tail -20 $OUT/${T}_pmc_fetch.log; exit 1; }
timeout -s KILL 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/${T}_pmc_write -o pmc --output-format csv -- python3 $R/bench.py $B --steps 2 --warmup 1 > $OUT/${T}_pmc_write.log 2>&1 || { echo "write pass failed rc=$?"; tail -20 $OUT/${T}_pmc_write.log; exit 1; }
cd $R
python3 tools/pmc_summary.py $OUT/${T}_prof $OUT/${T}_pmc_fetch $OUT/${T}_pmc_write $OUT/${T}_pmc_summary.json $OUT/${T}_prof.log
# the trace CSVs are large; keep only the stats and counter summaries (the check above read them)
find $OUT/${T}_prof $OUT/${T}_pmc_fetch $OUT/${T}_pmc_write -name "*kernel_trace.csv" -delete
ls -R $OUT | head -40
