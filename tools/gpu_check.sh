# GPU parity suite then a short bench (no CPU baseline / roofline); used while iterating
set -e
OUT=${OUT:-bench_out}  # where the logs go
mkdir -p "$OUT"
timeout -k 10 500 python -m pytest tests -m gpu -x -q > gpurun_out/t.log 2>&1
timeout -k 10 400 python bench.py --full --cpu-baseline 0 --roofline 0 "$@" > $OUT/bench.log 2>&1
