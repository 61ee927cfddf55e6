# Developer tool (GPU box): same-box A/B of two builds of the library on the headline workload. Put the OTHER build at
# rslqr_amd/librslqr_amd_prev.so first (tools/mk_prev.sh); the ctypes mirror loads it through NDLQR_LIBRARY. Boxes differ
# by +-4 %: only runs of one call compare.    bash tools/ab_prev.sh [bench.py arguments, e.g. --batch 1]
# Legs interleaved, each under its own time limit (LEG_TIMEOUT seconds); the first leg that fails ends the run.
set -o pipefail
for i in 1 2 3; do
for lib in prev new; do
  if [ $lib = prev ]; then export NDLQR_LIBRARY=$PWD/rslqr_amd/librslqr_amd_prev.so; else unset NDLQR_LIBRARY; fi
  timeout -k 10 ${LEG_TIMEOUT:-240} python bench.py --full --no-cpu --no-modes --no-configs --no-transfers --steps ${STEPS:-100} "$@" 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read()); ks=dict(d['roofline']['kernels']); ks[d['roofline']['kernel']]=d['roofline']
print('$lib', round(d['value']), round(d['ms_per_step'],4), round(d['pipeline']['ms_per_step_depth1'],4), {k:round(v['ms_per_step'],4) for k,v in sorted(ks.items())})" || exit 1
done; done
