#!/bin/bash
# One GPU session: full GPU tests, smoke, the full bench line (1 GPU), host path, kernel trace profile.
# usage: tools/gpu_round.sh [tag]   (results under $OUT, default bench_out/)
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
TAG=${1:-r01}
OUT=${OUT:-$R/bench_out}
mkdir -p $OUT
cd $R
timeout -k 10 900 python -m pytest tests -m gpu -x -q -p no:cacheprovider > $OUT/$TAG.tests.log 2>&1 || { echo TESTS_FAILED; tail -30 $OUT/$TAG.tests.log; exit 1; }
tail -2 $OUT/$TAG.tests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/$TAG.smoke.log 2>&1 || { echo SMOKE_FAILED; cat $OUT/$TAG.smoke.log; exit 1; }
tail -1 $OUT/$TAG.smoke.log
timeout -k 10 400 python bench.py --full > $OUT/$TAG.bench.json 2> $OUT/$TAG.bench.err || { echo BENCH_FAILED; tail $OUT/$TAG.bench.err; exit 1; }
cat $OUT/$TAG.bench.json
for b in 64 256 1024; do timeout -k 10 300 python tools/host_path_bench.py --batch $b >> $OUT/$TAG.hostpath.json 2>>$OUT/$TAG.hostpath.err || exit 1; done
cat $OUT/$TAG.hostpath.json
export TMPDIR=/tmp
cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$TAG.prof -- python3 $R/bench.py --no-cpu > $OUT/$TAG.prof.log 2>&1 || { echo PROF_FAILED; tail $OUT/$TAG.prof.log; exit 1; }
tail -1 $OUT/$TAG.prof.log
python3 $R/tools/prof_agree.py $OUT/$TAG.prof $OUT/$TAG.prof.log $OUT/$TAG.timing_agreement.json
echo ROUND_DONE
