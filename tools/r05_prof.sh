# Round-5 profile pass (run through gpurun from the repo root): the default bench line, a rocprofv3 kernel-trace
# stats run of a short bench (only the stats CSV kept: the trace itself exceeds what gpurun returns), and three PMC
# passes over eager cp_step launches (tools/pmc_cp_step.py).
set -e
OUT=${OUT:-bench_out}  # where the bench logs go (relative to the repo root)
R=$GRAFT_REPO_ROOT
mkdir -p $R/gpurun_out
cd $R
mkdir -p "$OUT"
timeout -k 10 600 python bench.py --full > $OUT/r05_bench.log 2>&1
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d /tmp/prof_bench -o run --output-format csv -- python3 $R/bench.py --full --steps 3 --warmup 1 --cpu-baseline 0 > $R/$OUT/r05_prof_bench.log 2>&1
find /tmp/prof_bench -name "*kernel_stats.csv" -exec cp {} $R/gpurun_out/r05_rocprof_bench_kernel_stats.csv \;
for i in 1 2 3; do
  C=$(echo "FETCH_SIZE WRITE_SIZE TCP_TCC_READ_REQ_sum" | cut -d' ' -f$i)
  timeout -s KILL 120 rocprofv3 --pmc $C -d $R/gpurun_out/pmc_cs$i -o run --output-format csv -- python3 $R/tools/pmc_cp_step.py > $R/gpurun_out/pmc$i.log 2>&1
done
for i in 1 2 3; do
  C=$(echo "FETCH_SIZE WRITE_SIZE TCP_TCC_READ_REQ_sum" | cut -d' ' -f$i)
  timeout -s KILL 180 rocprofv3 --pmc $C -d $R/gpurun_out/pmc_tt$i -o run --output-format csv -- python3 $R/tools/pmc_talker_tail.py > $R/gpurun_out/pmct$i.log 2>&1
done
echo done
