#!/bin/bash
# A/B: bench per library variant, alternated twice
set -o pipefail
R=$GRAFT_REPO_ROOT
O=${AB_OUT:-$R/ab_out}  # the runs' logs
mkdir -p "$O"
for rep in 1 2; do
for v in "" ${AB_VARIANTS}; do
  L=$R/building-gan-graph-conditioned-architectural-volume-generation_amd/vgan/libvgan_hip$v.so
  VGAN_LIB=$L timeout -k 10 120 python bench.py --full --no-stress --no-cpu-baseline --no-fresh --no-sweep --steps 30 > /dev/null 2> $O/ab_${v}_${rep}.err || exit 1
  echo "v=$v rep=$rep $(grep -E 'timed|aggregate_fwd|k_gemm16' $O/ab_${v}_${rep}.err | tr '\n' ' ')"
done
done
