set -o pipefail
R=$GRAFT_REPO_ROOT
O=${AB_OUT:-$R/ab_out}  # the runs' logs
mkdir -p "$O"
for rep in 1 2; do
for args in "--no-sweep --steps 20" "--no-sweep --steps 30" "--steps 20"; do
  timeout -k 10 200 python bench.py --full --no-stress --no-cpu-baseline --no-bf16 $args > /dev/null 2> $O/fab.err || exit 1
  echo "$args rep=$rep: $(grep -E 'timed \(|fresh batches|sweep f' $O/fab.err | sed 's/\[bench [0-9:]*\] //' | tr '\n' ' ')"
done
done
