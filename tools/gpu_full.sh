#!/bin/bash
# full GPU validation + benches (each leg bounded).   usage: tools/gpu_full.sh <outdir>  (relative to the repository root)
cd "$GRAFT_REPO_ROOT" || exit 1
O=${1:?usage: tools/gpu_full.sh <outdir>}; mkdir -p $O
timeout 1500 python -m pytest tests -m gpu -x -q > $O/pytest.log 2>&1; echo "pytest rc=$?"; tail -4 $O/pytest.log
for w in c2 10m parity64 c4shard; do
  timeout 400 python bench.py --full --workload $w --no-cpu-baseline > $O/bench_$w.json 2>$O/bench_$w.err
  python - "$w" "$O" <<'PY'
import json,sys
w, o = sys.argv[1], sys.argv[2]
try:
    d=json.loads([l for l in open(f"{o}/bench_{w}.json") if l.startswith("{")][-1])
    print(w, round(d["ms_per_step"],3), "ms", round(d["value"]/1e6,1), "M edges/s gate", round(d["roofline"]["avg_launch_ms"],4), "frac", round(d["roofline"]["frac"],3), "host", round(d["host_enqueue_ms_per_step"],2))
except Exception as ex:
    print(w, "FAILED", ex)
PY
done
timeout 400 python bench.py --full --mode train --steps 10 --warmup 3 --no-cpu-baseline > $O/bench_train.json 2>$O/bench_train.err
python - "$O" <<'PY'
import json,sys
try:
    d=json.loads([l for l in open(sys.argv[1] + "/bench_train.json") if l.startswith("{")][-1])
    print("train", round(d["ms_per_step"],2), "ms", round(d["value"]/1e6,2), "M edges/s host", round(d["host_enqueue_ms_per_step"],1))
except Exception as ex:
    print("train FAILED", ex)
PY
