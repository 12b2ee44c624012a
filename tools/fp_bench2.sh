set -e
OUT=${OUT:-bench_out}  # where the logs go
mkdir -p "$OUT"
timeout -k 10 500 python bench.py --full --cpu-baseline 0 --roofline 0 > $OUT/fpb_1.log 2>&1
timeout -k 10 500 python bench.py --full --cpu-baseline 0 --roofline 0 > $OUT/fpb_2.log 2>&1
QT_IM2COL_MAX_M=256 timeout -k 10 500 python bench.py --full --cpu-baseline 0 --roofline 0 > $OUT/fpb_3.log 2>&1
