#!/bin/bash
# A/B of environment settings on the fresh-batch leg: AB_ENVS="A=1 A=2" bash tools/fresh_env_ab.sh
# (several variables in one setting: comma-separated), alternated twice.
set -o pipefail
R=$GRAFT_REPO_ROOT
O=${AB_OUT:-$R/ab_out}  # the runs' logs
mkdir -p "$O"
for rep in 1 2; do
for e in ${AB_ENVS}; do
  env ${e//,/ } timeout -k 10 200 python bench.py --full --no-stress --no-cpu-baseline --no-sweep --no-bf16 --steps 30 > /dev/null 2> $O/fenv.err || exit 1
  echo "$e rep=$rep: $(grep -E 'timed \(|fresh batches' $O/fenv.err | sed 's/\[bench [0-9:]*\] //' | tr '\n' ' ')"
done
done
