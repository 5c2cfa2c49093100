#!/bin/bash
# k_map ablation timings (measurement only): WCG_MAP_ABLATE = 0 full, 5 input loads, 4 + staging
# and masks, 1 + start lists, 2 + the per-step first-entry reads and merges, 3 + the short-key
# decodes and probes (misses dropped); the levels are described above utf8_mask_list in wcg_map.h
for A in ${ABLATIONS:-0 1 2 3}; do
  WCG_MAP_ABLATE=$A python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-verify --no-end-to-end "$@" > /tmp/abl_$A.json || exit $?
  python3 - "$A" <<'PY'
import json, sys
d = json.loads(open(f"/tmp/abl_{sys.argv[1]}.json").read().strip().splitlines()[-1])
print(sys.argv[1], d["phase_ms_avg"], d.get("stats"))
PY
done
