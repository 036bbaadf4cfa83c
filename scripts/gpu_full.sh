# full round evidence: tests, smoke, default bench, rocprof kernel trace of the bench command, PMC traffic passes
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
export OUT=${OUT:-evidence}; mkdir -p $OUT   # where this script leaves its logs
timeout 500 python -m pytest tests -q -m gpu > $OUT/t1.log 2>&1; echo exit=$? >> $OUT/t1.log; tail -3 $OUT/t1.log
timeout 120 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; echo exit=$? >> $OUT/smoke.log; tail -2 $OUT/smoke.log
rm -rf $OUT/prof $OUT/pmc; mkdir -p $OUT/prof $OUT/pmc
timeout 300 rocprofv3 --kernel-trace --stats -d $OUT/prof -o r01 -- python bench.py --steps 1 --warmup 1 --num_steps 200 --no_cpu_baseline --no_roofline > $OUT/prof/run.log 2>&1; echo exit=$? >> $OUT/prof/run.log
tail -1 $OUT/prof/run.log
for c in FETCH_SIZE WRITE_SIZE; do
  timeout 300 rocprofv3 --pmc $c --kernel-trace -d $OUT/pmc -o pmc_$c -- python bench.py --steps 1 --warmup 0 --num_steps 40 --no_cpu_baseline --no_roofline > $OUT/pmc/run_$c.log 2>&1; echo "$c exit=$?" >> $OUT/pmc/run_$c.log; tail -1 $OUT/pmc/run_$c.log
done
f=$(find $OUT/prof -name "*_results.db" | head -1); python scripts/prof_summary.py $f > $OUT/prof_summary.txt 2>&1; head -12 $OUT/prof_summary.txt
python scripts/pmc_summary.py $(find $OUT/pmc -name "pmc_FETCH_SIZE*_results.db" | head -1) $(find $OUT/pmc -name "pmc_WRITE_SIZE*_results.db" | head -1) profiles/traffic_latest.json > $OUT/pmc_summary.txt 2>&1; cat $OUT/pmc_summary.txt | head -12
cp profiles/traffic_latest.json $OUT/traffic_latest.json
timeout 500 python bench.py --full > $OUT/bench_default.log 2>&1; echo exit=$? >> $OUT/bench_default.log; tail -2 $OUT/bench_default.log | cut -c1-900
# phase clocks need the stamp sites compiled in (the product library has none); the box is discarded afterwards
touch said_amd/csrc/gemm_common.h; SAID_EXTRA_DEFS=-DSAID_CLK_STAMPS python -m said_amd.build > /dev/null 2>&1
timeout 200 python scripts/debug_clocks.py > $OUT/clk.log 2>&1; grep -c "^launch" $OUT/clk.log
