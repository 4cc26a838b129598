#!/bin/bash
# rocprofv3 kernel-trace + stats of a short bench run (no PMC counters here).  PROF_OUT names the
# output directory (default prof_out/).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
O=${PROF_OUT:-prof_out}
mkdir -p $O/prof
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
timeout -k 10 ${PROF_TIMEOUT:-600} rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o run -- \
  python3 bench.py ${PROF_BENCH_ARGS:---full --steps 3 --warmup 1 --no-cpu-baseline --fwd-steps 1} > $O/prof_bench.log 2>&1
rc=$?
echo "rocprof rc=$rc"
tail -3 $O/prof_bench.log
find $O/prof -name "*stats*" | head
exit $rc
