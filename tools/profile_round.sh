#!/bin/bash
# Round-end measurement: bench line, rocprofv3 kernel stats, HBM counters (separate PMC passes).
# usage (on an MI355X host, from the repo root): bash tools/profile_round.sh <tag> <output dir>
tag=$1
O=$(realpath -m "${2:?usage: bash tools/profile_round.sh <tag> <output dir>}")
R=$GRAFT_REPO_ROOT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 python3 $R/bench.py --full --steps 50 --warmup 5 > $O/${tag}_bench.log 2>&1 || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/${tag}_prof -- python3 $R/bench.py --steps 50 --warmup 5 --no-cpu-baseline --no-pipeline > $O/${tag}_prof.log 2>&1 || exit 1
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 300 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $O/${tag}_pmc_$c -- python3 $R/bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-pipeline > $O/${tag}_pmc_$c.log 2>&1 || exit 1
done
tail -1 $O/${tag}_bench.log
