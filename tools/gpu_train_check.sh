#!/bin/bash
# training tests + training bench.   usage: tools/gpu_train_check.sh <outdir>  (relative to the repository root)
cd "$GRAFT_REPO_ROOT" || exit 1
O=${1:?usage: tools/gpu_train_check.sh <outdir>}; mkdir -p $O
timeout 900 python -m pytest tests/test_hip_training.py tests/test_hip_partition.py -x -q 2>&1 | tail -15
timeout 300 python bench.py --full --mode train --steps 10 --warmup 3 --no-cpu-baseline > $O/train_now.json 2>$O/train_now.err; tail -c 700 $O/train_now.json
