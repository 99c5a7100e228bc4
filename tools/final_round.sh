#!/bin/bash
# The closing GPU visit of a round, run AFTER the last source commit: the whole GPU suite inside the driver's window (it FAILS when
# the suite needs more than 700 s), smoke, the full bench line of both modes.  Outputs under $OUT_DIR (default bench_out/);
# profiles/rNN_gpu_suite_summary.txt is made from them (tail of the pytest log incl. --durations=30).
R=$(cd "$(dirname "$0")/.." && pwd)
O=${OUT_DIR:-$R/bench_out}
cd $R
mkdir -p $O
export TMPDIR=/tmp
rm -f */test_durations.tsv */native_solve_timings.tsv   # earlier runs' share of what tests/conftest.py and tests/test_distributed.py append to
LIMIT=${SUITE_LIMIT:-700}
t0=$(date +%s)
{ time timeout 1150 python -m pytest tests -m gpu -q --durations=30 ; } > $O/pytest_gpu.log 2>&1
rc=$?
t1=$(date +%s)
echo "pytest exit $rc, $((t1 - t0)) s wall (limit $LIMIT s)" >> $O/pytest_gpu.log
{ time timeout 300 python -c "import __graft_entry__ as g; g.smoke()" ; } > $O/smoke.log 2>&1
{ time timeout 900 python bench.py --full ; } > $O/bench.json 2> $O/bench.err
{ time timeout 300 python bench.py --full --solver gamg ; } > $O/bench_gamg.json 2> $O/bench_gamg.err
grep -E "passed|failed|pytest exit" $O/pytest_gpu.log; tail -2 $O/smoke.log; cut -c1-700 $O/bench.json; cut -c1-300 $O/bench_gamg.json
if [ $rc -ne 0 ] || [ $((t1 - t0)) -gt $LIMIT ]; then echo "FINAL ROUND: the GPU suite failed or exceeded $LIMIT s"; exit 1; fi
