#!/bin/bash
# Where do k_gather<16>'s 3.9 us between "alone" and "in the step" go?  L2 counters and kernel times of the default bench
# command and of tools/experiments/xcd_place/gather_alone.py in its three modes.  Counters and the kernel trace never
# share a run; TCC_HIT / TCC_MISS in one run, TCC_EA0_RDREQ (gfx950's name of the L2's memory-side read requests) in
# another.  Every step has a time limit of its own and the script stops at the first step that fails.
#   bash tools/experiments/xcd_place/profile.sh OUTDIR
set -e -o pipefail
R=$(cd "$(dirname "$0")/../../.." && pwd)
out=$(mkdir -p "$1" && cd "$1" && pwd)
cd /tmp; export TMPDIR=/tmp
prof() {    # run name, rest: the command
  local run=$1; shift
  timeout -k 10 150 rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --output-format csv -d $out/${run}_pmc_hit -- "$@" > $out/${run}_pmc_hit.log 2>&1
  timeout -k 10 150 rocprofv3 --pmc TCC_EA0_RDREQ_sum --output-format csv -d $out/${run}_pmc_rdreq -- "$@" > $out/${run}_pmc_rdreq.log 2>&1
  timeout -k 10 150 rocprofv3 --kernel-trace --stats --output-format csv -d $out/${run}_trace -- "$@" > $out/${run}_trace.log 2>&1
  echo "$run done"
}
prof step python3 $R/bench.py --gpus 1 --steps 20 --warmup 2
prof static python3 $R/tools/experiments/xcd_place/gather_alone.py static
prof pair python3 $R/tools/experiments/xcd_place/gather_alone.py pair
prof copy python3 $R/tools/experiments/xcd_place/gather_alone.py copy
python3 $R/tools/experiments/xcd_place/reduce.py $out $out/xcd_pmc.tsv $out/xcd_times.tsv
cat $out/xcd_times.tsv $out/xcd_pmc.tsv
