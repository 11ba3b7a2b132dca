#!/bin/bash
# One GPU-box session, parameterised.  Usage (repo root on the GPU box): bash tools/gpu_session.sh <tag> <step> [<step> ...]
# Logs go to $OUT (default measure_out/ at the repository root).
#   tests[:<pytest -k expr>]  parity suite with -s (measured values kept), per-test timeout; log -> $OUT/pytest_<tag>.log
#   smoke                     __graft_entry__.smoke()
#   bench                     python bench.py --full (fewer steps)                      -> $OUT/bench_<tag>.log
#   prof                      rocprofv3 kernel stats of the infer step alone (no train line, one stream, no graph)
#   proftrain[:<batch>]       rocprofv3 kernel stats of the training step
#   gemm[:<scheds>]           tools/gemm_probe.py A/B of the conv256 schedules on the bench shapes (with and without fused sums)
#   run:<command>             anything else, output -> $OUT/run_<tag>.log
TAG=${1:-r}; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
export OUT=${OUT:-$ROOT/measure_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
for STEP in "$@"; do
  case "$STEP" in
    tests*)
      K="${STEP#tests}"; K="${K#:}"
      if [ -n "$K" ]; then
        timeout 900 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider -s --timeout 200 --timeout-method thread -k "$K" > $OUT/pytest_$TAG.log 2>&1
      else
        timeout 1100 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider -s --timeout 200 --timeout-method thread > $OUT/pytest_$TAG.log 2>&1
      fi
      echo "pytest rc=$?"; grep -E "passed|failed|error|Timeout" $OUT/pytest_$TAG.log | tail -n 5
      grep -E "^(FAILED|ERROR)" $OUT/pytest_$TAG.log | head -n 40 ;;
    smoke)
      timeout 240 python __graft_entry__.py smoke > $OUT/smoke_$TAG.log 2>&1; echo "smoke rc=$?"; tail -n 4 $OUT/smoke_$TAG.log ;;
    bench)
      timeout 500 python bench.py --steps 100 --warmup 10 --full > $OUT/bench_$TAG.log 2>&1; echo "bench rc=$?"; tail -n 2 $OUT/bench_$TAG.log | cut -c 1-3500 ;;
    prof)
      (cd /tmp && timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_$TAG -o bench -- python $ROOT/bench.py --steps 20 --warmup 3 --graph 0 --streams 1 --no-cpu-baseline --no-roofline --no-train-line > $OUT/prof_$TAG.log 2>&1)
      echo "rocprof rc=$?"; find /tmp/prof_$TAG -name "*kernel_stats.csv" | head -n 1 | xargs -I{} cp {} $OUT/kernel_stats_$TAG.csv
      head -n 32 $OUT/kernel_stats_$TAG.csv | cut -c 1-160 ;;
    proftrain*)
      GB="${STEP#proftrain}"; GB="${GB#:}"; GB=${GB:-256}
      (cd /tmp && timeout 500 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/proft_$TAG -o tr -- python $ROOT/bench.py --mode train --global-batch $GB --steps 10 --warmup 5 > $OUT/proftrain_${TAG}_b$GB.log 2>&1)
      echo "rocprof train rc=$?"; find /tmp/proft_$TAG -name "*kernel_stats.csv" | head -n 1 | xargs -I{} cp {} $OUT/kernel_stats_train_${TAG}_b$GB.csv
      grep -h '^{"metric"' $OUT/proftrain_${TAG}_b$GB.log | cut -c1-500; head -n 24 $OUT/kernel_stats_train_${TAG}_b$GB.csv | cut -c 1-150 ;;
    gemm*)
      S="${STEP#gemm}"; S="${S#:}"; S=${S:-4,5,6}
      timeout 300 python tools/gemm_probe.py 5 $S 1536x1536 512x512 > $OUT/gemm_$TAG.log 2>&1
      PSUM=1 timeout 300 python tools/gemm_probe.py 5 $S 1536x1536 512x512 >> $OUT/gemm_$TAG.log 2>&1
      echo "gemm rc=$?"; cat $OUT/gemm_$TAG.log ;;
    run:*)
      CMD="${STEP#run:}"; timeout 600 bash -c "$CMD" > $OUT/run_$TAG.log 2>&1; echo "run rc=$?"; tail -n 30 $OUT/run_$TAG.log | cut -c 1-400 ;;
  esac
done
