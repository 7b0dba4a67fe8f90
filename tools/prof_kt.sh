# Kernel trace of one whole default bench run (every leg); output $OUT_DIR/ktg (default out/ktg in the repository).
R=$(cd "$(dirname "$0")/.." && pwd)
OUT_DIR=${OUT_DIR:-$R/out}
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT_DIR/ktg" -o kt -- python3 "$R/bench.py" --full --steps 20 --warmup 5
