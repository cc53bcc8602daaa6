#!/bin/bash
# round 6: the whole GPU suite + the driver's bench invocation + the tracker A/B
cd $GRAFT_REPO_ROOT
mkdir -p gpurun_out/r06
timeout 2400 python -m pytest tests/ -x -q -m gpu 2>&1 | tail -8 | tee gpurun_out/r06/pytest_gpu.log
timeout 900 python bench.py --full 2>/dev/null; echo "bench rc $?"   # the line on stdout, the full result in bench_extras.json
LIBS="lib lib_exp_nosched" bash scripts/gpu_r6_tracker.sh 2>&1 | grep -v "^{" | tail -12
