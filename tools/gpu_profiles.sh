# Profiles on an MI355X, from the repository root: rocprofv3 kernel stats of the bwa-sr-1 task
# phase (the rooflines' kernels, bench.py --full --task-only) and of the correction loop, then
# the PMC FETCH_SIZE / WRITE_SIZE passes of the task phase; outputs under $OUT (default
# prof_out/), prefix $1
set -e
export OUT=${OUT:-prof_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
P=${1:-p}
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/${P}_task" -o run --output-format csv -- python3 bench.py --full --task-only --steps 3 --warmup 1 --no-cpu-baseline > "$OUT/${P}_task.json" 2> "$OUT/${P}_task.err"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/${P}_loop" -o run --output-format csv -- python3 bench.py --loop-only --steps 2 --warmup 1 > "$OUT/${P}_loop.json" 2> "$OUT/${P}_loop.err"
bash tools/pmc.sh
