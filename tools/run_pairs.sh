#!/bin/bash
# parity tests, then same-box comparisons of the paired data-gradient / weight-gradient launches of the 16x16 and 8x8 layers:
# the default against ARVAE_NO_PAIR32=1 (two launches per layer)
cd "$(dirname "$0")/.."
mkdir -p gpurun_out
python -m pytest tests/test_hip_parity.py -x -q -m gpu 2>&1 | tail -4 > gpurun_out/pairs_tests.txt
q() { python -c 'import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(round(d["value"]), round(d["ms_per_step"],4))'; }
{
for rep in 1 2; do
  echo "paired (default)  $(python bench.py --full --no-cpu-baseline --no-secondary 2>/dev/null | q)"
  echo "two launches      $(ARVAE_NO_PAIR32=1 python bench.py --full --no-cpu-baseline --no-secondary 2>/dev/null | q)"
done
} > gpurun_out/pairs_bench.txt 2>&1
bash tools/trace_kernels.sh all > gpurun_out/pairs_trace.txt 2>&1
