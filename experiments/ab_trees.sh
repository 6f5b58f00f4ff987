#!/bin/bash
# experiments/ab_trees.sh REPS DIR...   (on the GPU box): alternate `bench.py --full` runs between built checkouts of the project (e.g. one
# of the parent commit and "." for this tree; BENCH_ARGS="--frames 81 --batch 128" etc. reach bench.py).  One line per run: the F16X3
# headline, the bf16_mode leg and that leg's qkv / attention kernel times -- the comparison a change of the bf16 flow is decided by.
# Each run under its own time limit; the first failure ends the script.
reps=$1; shift
for r in $(seq $reps); do
  for d in "$@"; do
    (cd "$d" && timeout -k 10 300 python bench.py --gpus 1 --steps 3 --warmup 1 --full --no-cpu-baseline --no-selfcheck --no-extras $BENCH_ARGS 2>/dev/null) | python -c "
import sys, json
d = json.loads(sys.stdin.read()); b = d['bf16_mode']; k = b['by_kernel_ms_per_step']
print('%-22s round $r  f16x3 %8.2f seq/s | bf16 %8.2f seq/s  attn %.1f/%.1f  qkv_sattn %.1f  qkv_tattn %.1f ms' % ('$d', d['value'], b['value'], k.get('attn_spatial', 0), k.get('attn_temporal', 0), k.get('qkv_sattn', 0), k.get('qkv_tattn', 0)))" || exit 1
  done
done
