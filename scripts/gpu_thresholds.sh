#!/bin/bash
cd $GRAFT_REPO_ROOT
for P in 5000 8000 12000 20000 30000; do
  for two_stage in 96 100000; do
    DSOPP_HIP_TWO_STAGE_MIN_CHUNKS=$two_stage python scripts/threshold_sweep.py 7 $P 2>/dev/null | grep "us per"
  done
done
for two_stage in 96 100000; do
  DSOPP_HIP_TWO_STAGE_MIN_CHUNKS=$two_stage python scripts/threshold_sweep.py 12 50000 1 2>/dev/null | grep "us per"
done
