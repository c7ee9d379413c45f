cd "$(dirname "$0")/.." || exit 1; export TMPDIR=/tmp; O=${1:?usage: tools/prof_c4.sh <outdir>  (relative to the repository root)}; mkdir -p $O
timeout 400 rocprofv3 --kernel-trace --stats -d $O -o r01 -- python bench.py --full --workload c4shard --steps 5 --warmup 2 --no-cpu-baseline --no-kernel-timers > $O/bench.json 2> $O/err.log
DB=$(find $O -name "*.db" | head -1); python tools/rocpd_summary.py "$DB" | head -14; find $O -name "*.db" -delete
