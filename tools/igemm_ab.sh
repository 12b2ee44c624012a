set -e
OUT=${OUT:-bench_out}  # where the logs go
mkdir -p "$OUT"
timeout -k 10 600 python -m pytest tests -m gpu -x -q > gpurun_out/t.log 2>&1
timeout -k 10 300 python tools/codec_bench.py > gpurun_out/codec.log 2>&1
QT_NO_IGEMM=1 timeout -k 10 300 python tools/codec_bench.py >> gpurun_out/codec.log 2>&1
timeout -k 10 400 python bench.py --full --cpu-baseline 0 --roofline 0 > $OUT/bench.log 2>&1
