#!/bin/bash
# Alternating C4 generate runs of two libraries (decode A/B):
#   bash tools/gen_ab.sh <tag> <lib_a> <lib_b> [rounds] [modes]     (modes: as bench_generate.py --modes)
set -o pipefail
tag=${1:?tag}; a=${2:?lib a}; b=${3:?lib b}; n=${4:-3}; modes=${5:-beam5,greedy}
out=gpurun_out/$tag; mkdir -p "$out"
lim=120; [ "$modes" != beam5,greedy ] && lim=300
for r in $(seq 1 "$n"); do
  for arm in a b; do
    lib=$a; [ $arm = b ] && lib=$b
    CAPGEN_LIB_PATH=$lib timeout -k 10 $lim python -u tools/bench_generate.py --reps 5 --modes "$modes" > "$out/gen_${arm}_$r.jsonl" 2>/dev/null || { echo "rc $? ($arm round $r)"; exit 1; }
    echo "$arm round $r: $(python -c "import json,sys;print(' '.join(f\"{json.loads(l)['metric'].split()[1]} {json.loads(l)['ms_per_batch']}\" for l in open('$out/gen_${arm}_$r.jsonl') if l.startswith('{')))")"
  done
done
