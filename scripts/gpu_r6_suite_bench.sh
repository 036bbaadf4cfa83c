cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
export OUT=${OUT:-evidence}; mkdir -p $OUT   # where this script leaves its logs
mkdir -p $OUT/s1
timeout 1200 python -m pytest tests -m gpu -q -x --durations=10 > $OUT/s1/suite.log 2>&1; echo "suite exit=$?" | tee -a $OUT/s1/suite.log
tail -15 $OUT/s1/suite.log
timeout 600 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/s1/bench_driver_like.log 2>&1; echo "bench exit=$?"
tail -1 $OUT/s1/bench_driver_like.log | cut -c1-400
