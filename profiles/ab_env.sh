#!/bin/bash
# A/B of ENVIRONMENT variants of the product library on ONE device (one gpurun call): alternating bench runs.
#   bash profiles/ab_env.sh <rounds> <name>=<ENV=VAL[,ENV=VAL...]|-> ...      ("-" = no extra environment)
# the launch-plan options travel in ONE variable whose pairs are joined by ":" (sfh_amd.options), e.g.
#   bash profiles/ab_env.sh 3 base=- two=SFH_OPTIONS=fuse_inc=0 both=SFH_OPTIONS=fuse_inc=0:up_single=4,SFH_PRECISION=bf16x6
# prints value / ms per step / unpipelined ms / per-group ms for every run
# (bench.py --full: the unpipelined pass and kernel_groups are not in a plain run; results go to $OUT, default bench_runs/)
R=$1; shift
export OUT=${OUT:-bench_runs}
mkdir -p $OUT
for i in $(seq 1 $R); do
  for spec in "$@"; do
    name=${spec%%=*}; envs=${spec#*=}
    if [ "$envs" = "-" ]; then envs=""; fi
    ( for kv in ${envs//,/ }; do export "$kv"; done
      python bench.py --full --no-cpu-baseline --no-extra-configs --steps 20 > $OUT/abe_${name}_$i.json 2>> $OUT/abe.err ) || exit 1
  done
done
python - "$@" <<'PY'
import json, glob, os, sys
for spec in sys.argv[1:]:
    name = spec.split("=")[0]
    for f in sorted(glob.glob(os.path.join(os.environ["OUT"], f"abe_{name}_*.json"))):
        d = json.loads(open(f).read().strip().splitlines()[-1])
        u = d["roofline"].get("unpipelined", {})
        print(f"{name:12s} {d['value']:8.2f} fps {d['ms_per_step']:7.3f} ms | predict() {u.get('ms_per_step')} ms", {k: v["ms_per_step"] for k, v in d["kernel_groups"].items()})
PY
