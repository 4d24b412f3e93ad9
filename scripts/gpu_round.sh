#!/bin/bash
# One GPU session: gpu tests, smoke, bench, rocprof kernel stats + HBM PMC passes.  Outputs -> gpurun_out/
set -x
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd /root/repo
mkdir -p gpurun_out
mkdir -p results      # bench.py's lines write here
export TMPDIR=/tmp
timeout 1500 python -m pytest tests -x -q -m gpu > gpurun_out/pytest_gpu.log 2>&1; echo "pytest rc=$?" | tee -a gpurun_out/pytest_gpu.log
tail -5 gpurun_out/pytest_gpu.log
timeout 300 python __graft_entry__.py --smoke > gpurun_out/smoke.log 2>&1; echo "smoke rc=$?"; tail -3 gpurun_out/smoke.log
timeout 900 python bench.py --full > results/bench.json 2> results/bench.err; echo "bench rc=$?"; cat results/bench.json; tail -3 results/bench.err
timeout 900 python bench.py --full --precision 64 --no-cpu-baseline > results/bench_f64.json 2> results/bench_f64.err; echo "bench f64 rc=$?"; cat results/bench_f64.json
R=$(pwd)
cd /tmp
timeout 600 rocprofv3 --kernel-trace --stats -d $R/results/prof -o r01 -- python $R/bench.py --full --steps 200 --warmup 20 --no-cpu-baseline --parity-steps 0 > $R/results/prof_bench.json 2> $R/results/prof.err; echo "rocprof rc=$?"
timeout 600 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $R/results/pmc_fetch -o f --output-format csv -- python $R/bench.py --full --steps 200 --warmup 20 --no-cpu-baseline --parity-steps 0 > /dev/null 2>> $R/results/prof.err; echo "pmc fetch rc=$?"
timeout 600 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $R/results/pmc_write -o w --output-format csv -- python $R/bench.py --full --steps 200 --warmup 20 --no-cpu-baseline --parity-steps 0 > /dev/null 2>> $R/results/prof.err; echo "pmc write rc=$?"
ls $R/results/prof $R/results/pmc_fetch $R/results/pmc_write | head -20
