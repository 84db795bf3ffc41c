#!/bin/bash
# Profile session of one round: every GPU step under its own time limit; stop
# at the first crash / timeout.  Outputs under bench_out/$ROUND/ (the
# summaries are copied to profiles/$ROUND/ afterwards; trace csvs dropped).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
# cooperative grids launched plainly after the same co-residency check:
# rocprofv3 segfaults at teardown after any cooperative launch (kg_common.hpp)
export KORALI_AMD_PLAIN_LAUNCH=1
R=$PWD
O=$R/bench_out/${ROUND:-r3}
mkdir -p $O
step() {
  local name=$1 secs=$2; shift 2
  echo "=== $name: $*" | tee -a "$O/steps.log"
  (cd /tmp && timeout -k 10 "$secs" "$@") > "$O/$name.log" 2>&1
  local rc=$?
  echo "=== $name rc=$rc" | tee -a "$O/steps.log"
  tail -3 "$O/$name.log"
  if [ $rc -ge 124 ] || [ $rc -eq 134 ] || [ $rc -eq 139 ]; then echo "FATAL step $name rc=$rc"; exit $rc; fi
  return 0
}
for s in ${STEPS:-tests}; do
  case $s in
    tests) step tests 1000 python -u -m pytest $R/tests -x -v -m gpu --timeout 300 --timeout-method thread -p no:cacheprovider --rootdir $R ;;
    avail) step avail 60 rocprofv3 --list-avail ;;
    bench) step bench 300 python $R/bench.py --full --steps 200 --warmup 10 ;;
    c3) step c3 400 python $R/bench.py --full --workload c3 --steps 40 --warmup 3 ;;
    c4) step c4 400 python $R/bench.py --full --workload c4 --steps 20 --warmup 3 ;;
    prof) step prof 300 rocprofv3 --kernel-trace --stats -d $O/prof_c2 -o run --output-format csv -- python $R/bench.py --full --steps 50 --warmup 5 --no-cpu-baseline ;;
    profc3) step profc3 300 rocprofv3 --kernel-trace --stats -d $O/prof_c3 -o run --output-format csv -- python $R/bench.py --full --workload c3 --steps 20 --warmup 2 --no-cpu-baseline ;;
    profc4) step profc4 300 rocprofv3 --kernel-trace --stats -d $O/prof_c4 -o run --output-format csv -- python $R/bench.py --full --workload c4 --steps 10 --warmup 2 --no-cpu-baseline ;;
    pmcf) step pmcf 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $O/pmc_fetch -o run --output-format csv -- python $R/bench.py --full --steps 20 --warmup 2 --no-cpu-baseline ;;
    pmcw) step pmcw 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $O/pmc_write -o run --output-format csv -- python $R/bench.py --full --steps 20 --warmup 2 --no-cpu-baseline ;;
    pmcm) step pmcm 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F64 GRBM_GUI_ACTIVE --kernel-trace -d $O/pmc_mfma -o run --output-format csv -- python $R/bench.py --full --steps 20 --warmup 2 --cov mfma --no-cpu-baseline ;;
    pmcf3) step pmcf3 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $O/pmc_fetch_c3 -o run --output-format csv -- python $R/bench.py --full --workload c3 --steps 12 --warmup 1 --no-cpu-baseline ;;
    pmcw3) step pmcw3 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $O/pmc_write_c3 -o run --output-format csv -- python $R/bench.py --full --workload c3 --steps 12 --warmup 1 --no-cpu-baseline ;;
    pmcf4) step pmcf4 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $O/pmc_fetch_c4 -o run --output-format csv -- python $R/bench.py --full --workload c4 --steps 4 --warmup 1 --no-cpu-baseline ;;
    pmcw4) step pmcw4 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $O/pmc_write_c4 -o run --output-format csv -- python $R/bench.py --full --workload c4 --steps 4 --warmup 1 --no-cpu-baseline ;;
    trace2) step trace2 200 env KORALI_AMD_TRACE_EIGEN=1 python $R/tools/trace_c2.py ;;
    trace4) step trace4 300 env KORALI_AMD_TRACE_EIGEN=1 python $R/tools/trace_c4.py ;;
    dist) step dist 700 python -u -m pytest $R/tests/test_gpu_distributed.py -x -v --timeout 300 --timeout-method thread -p no:cacheprovider --rootdir $R ;;
    engvr) step engvr 500 python -u -m pytest $R/tests/test_gpu_engine.py -x -v -k vracer --timeout 300 --timeout-method thread -p no:cacheprovider --rootdir $R ;;
    vrtests) step vrtests 400 python -u -m pytest $R/tests/test_gpu_vracer.py -x -v --timeout 200 --timeout-method thread -p no:cacheprovider --rootdir $R ;;
    c5) step c5 300 python $R/bench.py --full --workload c5 --steps 10 --warmup 2 ;;
    profc5) step profc5 300 rocprofv3 --kernel-trace --stats -d $O/prof_c5 -o run --output-format csv -- python $R/bench.py --full --workload c5 --steps 2 --warmup 0 --no-cpu-baseline ;;
    pmcf5) step pmcf5 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $O/pmc_fetch_c5 -o run --output-format csv -- python $R/bench.py --full --workload c5 --steps 2 --warmup 0 --no-cpu-baseline ;;
    pmcw5) step pmcw5 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $O/pmc_write_c5 -o run --output-format csv -- python $R/bench.py --full --workload c5 --steps 2 --warmup 0 --no-cpu-baseline ;;
    pmcm4) step pmcm4 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F64 GRBM_GUI_ACTIVE --kernel-trace -d $O/pmc_mfma_c4 -o run --output-format csv -- python $R/bench.py --full --workload c4 --steps 5 --warmup 1 --no-cpu-baseline ;;
  esac
done
find $O -name "*kernel_trace.csv" ! -path "*prof_c2*" -delete
echo "session done"
