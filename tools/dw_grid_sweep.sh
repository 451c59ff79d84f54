#!/bin/bash
# step time against the grouped (weight-gradient) grid cap, CAPGEN_DW_GRID workgroups (0 = one per CU):
# alternating rounds of every arm in one session (tools/ab.py).  Run from the repo root on the GPU box.
#   bash tools/dw_grid_sweep.sh [rounds] [caps...]
set -o pipefail
rounds=${1:-4}
[ $# -gt 0 ] && shift
caps=("$@")
[ ${#caps[@]} -gt 0 ] || caps=(192 320 128)
args=(--arm "cap256:")
for c in "${caps[@]}"; do args+=(--arm "cap$c:CAPGEN_DW_GRID=$c"); done
timeout -k 10 1100 python -u tools/ab.py --rounds "$rounds" --steps 200 "${args[@]}"
