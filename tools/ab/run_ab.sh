#!/bin/bash
# A/B of solver library builds on ONE box: bash tools/ab/run_ab.sh libA.so libB.so ...  (paths relative to the repo root; "cur" = the in-tree build)
# The builds alternate, REPS times (default 2); every run has its own time limit and the first one that fails ends the comparison.
set -u -o pipefail
for rep in $(seq 1 ${REPS:-2}); do
for lib in "$@"; do
  if [ "$lib" = "cur" ]; then unset UVS_SOLVER_LIB; else export UVS_SOLVER_LIB=$PWD/$lib; fi
  timeout -k 10 300 python bench.py --steps 20 --warmup 3 --full --no-cpu-baseline --no-replay --no-large --no-stream 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('$lib', 'batch ms %.4f (kernel %.4f) value %.0f  single %.4f ms' % (d['ms_per_step'], d['roofline']['kernel_ms_per_launch'], d['value'], d['single_window_ms']))" || { echo "$lib: run failed, stopping"; exit 1; }
done; done
