#!/bin/bash
# one GPU-box visit: tests, default bench, N>1 plumbing checks.  Every leg bounded.   usage: tools/gpu_round.sh <outdir>  (relative to the repository root)
cd "$GRAFT_REPO_ROOT" || exit 1
O=${1:?usage: tools/gpu_round.sh <outdir>}; mkdir -p $O
timeout 1500 python -m pytest tests -m gpu -x -q > $O/pytest.log 2>&1; echo "pytest rc=$?" | tee -a $O/pytest.log
tail -5 $O/pytest.log
timeout 400 python bench.py --full > $O/bench_default.json 2> $O/bench_default.err; echo "bench rc=$?"
tail -c 600 $O/bench_default.json
for mode in infer train; do
  timeout 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --full --gpus 2 --steps 5 --warmup 2 --mode $mode --one-gpu-gloo > $O/bench_n2_$mode.json 2> $O/bench_n2_$mode.err; echo "n2 $mode rc=$?"
  tail -c 400 $O/bench_n2_$mode.json; tail -5 $O/bench_n2_$mode.err
done
timeout 400 python bench.py --full --mode train --steps 10 --warmup 3 > $O/bench_train.json 2> $O/bench_train.err; echo "train rc=$?"
tail -c 300 $O/bench_train.json
