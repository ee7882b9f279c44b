#!/bin/bash
# Runs on the GPU box: rocprofv3 kernel trace + stats of the headline bench (--full: the standalone applyJTJ launches too), then FETCH_SIZE and
# WRITE_SIZE in separate --pmc passes (the TCC counter slots do not fit both).  Everything lands in $PROFILE_OUT (default profile_out/).
set -e              # a failed or timed-out run ends the script
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=$(realpath -m "${PROFILE_OUT:-$R/profile_out}")
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_kt -- python3 $R/bench.py --full --no-cpu-baseline --no-small > $O/prof_kt.log 2>&1
timeout 400 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/prof_fetch -- python3 $R/bench.py --full --no-cpu-baseline --no-small --steps 2 --warmup 1 > $O/prof_fetch.log 2>&1
timeout 400 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/prof_write -- python3 $R/bench.py --full --no-cpu-baseline --no-small --steps 2 --warmup 1 > $O/prof_write.log 2>&1
cd $R
grep "^{" $O/prof_kt.log | tail -1 > $O/bench_under_rocprof.json
timeout 400 python3 bench.py --full > $O/bench_plain.log 2>&1
grep "^{" $O/bench_plain.log | tail -1 > $O/bench_plain.json
ls -R $O | head -40
