set -e
OUT=${OUT:-bench_out}  # where the logs go
mkdir -p "$OUT"
timeout -k 10 500 python -m pytest tests -m gpu -x -q > gpurun_out/t.log 2>&1
for g in 1 2 4; do
  timeout -k 10 300 python bench.py --full --cpu-baseline 0 --roofline 0 --row-groups $g > $OUT/bench_g$g.log 2>&1
done
