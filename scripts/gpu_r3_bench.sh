# round 3: the default bench line (headline + secondary configurations)
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
export OUT=${OUT:-evidence}; mkdir -p $OUT   # where this script leaves its logs
mkdir -p $OUT
timeout 900 python bench.py --steps 5 --warmup 2 --full > $OUT/r3_bench_default.log 2>&1
echo "exit=$?" >> $OUT/r3_bench_default.log
tail -c 6000 $OUT/r3_bench_default.log
