#!/bin/bash
# slant_up time per library variant (timing probes; results of probes are wrong)
# Writes probe_<config>_<variant>.json under $OUT (default: bench_out).
set -o pipefail
CFG=${1:-hd256}; shift
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for v in "$@"; do
  lib=stereo_matching_amd/libsgm_hip.so; [ "$v" != base ] && lib=build/$v/libsgm_hip.so
  SGM_SLANT=1 SGM_HIP_LIB=$lib timeout -k 10 300 python bench.py --full --config $CFG --steps 6 --warmup 2 --no-cpu-baseline > $OUT/probe_${CFG}_$v.json 2>/dev/null || exit 1
  python3 -c "
import json; r=json.load(open('$OUT/probe_${CFG}_$v.json')); k=r['kernels']
print('%-10s %-8s step %8.3f ms  slant_up %8.1f us' % ('$CFG', '$v', r['ms_per_step'], k['slant_up']['avg_us']), 'down %8.1f' % k.get('slant_down',{}).get('avg_us',0))"
done
