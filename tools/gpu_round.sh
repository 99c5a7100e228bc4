#!/bin/bash
# one visit to a GPU box: tests, smoke, the full bench line, sweep, rocprof (outputs under $OUT_DIR, default bench_out/)
R=$(cd "$(dirname "$0")/.." && pwd)
O=${OUT_DIR:-$R/bench_out}
cd $R
mkdir -p $O
export TMPDIR=/tmp
{ time timeout 900 python -m pytest tests -m gpu -x -q ; } > $O/pytest_gpu.log 2>&1
echo "pytest exit $?" >> $O/pytest_gpu.log
{ time timeout 300 python -c "import __graft_entry__ as g; g.smoke()" ; } > $O/smoke.log 2>&1
{ time timeout 600 python bench.py --full --steps 200 --warmup 10 ; } > $O/bench.json 2> $O/bench.err
if [ -n "$DO_SWEEP" ]; then { time timeout 900 python tools/sweep.py ; } > $O/sweep.log 2>&1 ; fi
if [ -n "$DO_PROF" ]; then
  cd /tmp
  timeout 600 rocprofv3 --kernel-trace --stats -d $O/prof -o bench -- python $R/bench.py --steps 100 --warmup 10 > $O/prof_bench.json 2> $O/prof_bench.err
  cd $R
  find $O/prof -name "*.db" -size +20M -delete 2>/dev/null
  ls -la $O/prof/* > $O/prof_ls.txt 2>&1
fi
tail -5 $O/pytest_gpu.log; cat $O/smoke.log | tail -3; cat $O/bench.json; tail -3 $O/bench.err
