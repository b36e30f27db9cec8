#!/bin/bash
# Stage 1: how many levels of the colour-table backward merge same-cell runs of consecutive covered pixels (N2M_BIN_MERGE_LEVELS, default 9).
O=${OUT_DIR:-bench_runs}/${1:-s1m}; mkdir -p $O
for m in 9 11 12 13 14 16; do
  N2M_BIN_MERGE_LEVELS=$m python bench.py --full --stage 1 --steps 60 --warmup 10 --no-cpu-baseline > $O/s1_m$m.json 2>/dev/null
  python - $m $O/s1_m$m.json <<'PY'
import json, sys
d = json.load(open(sys.argv[2]))
k = d["kernels"]
print(f"merge levels {sys.argv[1]:>2s}: {d['ms_per_step']:.3f} ms/step   colour-table backward {k['grid_encode_backward']['avg_us']:.1f} us   lookup {k['grid_encode_forward']['avg_us']:.1f}")
PY
done
