#!/bin/bash
# experiments/attn_x3_tile_ab.sh PARENT_LIB [REPS=5] [OUT=profiles/attn_${TABLE}_ab.json] [TABLE=x3_tile]   (on the GPU box)
# Alternates the parent commit's build of libd3d_hip.so (PARENT_LIB) and the in-tree build, REPS times each, one process per leg
# (experiments/attn_x3_tile_ab.py leg TABLE), and collects the per-launch times of the attention kernels of the shape table TABLE
# (x3_tile: the kernels built on attn_x3_tile.h; f32_tile: those on attn_f32_tile.h).
# Stops at the first leg that fails; the in-tree library is put back in every case.
parent=$1; reps=${2:-5}; table=${4:-x3_tile}; out=${3:-profiles/attn_${table}_ab.json}
cur=diff3dhpe_amd/libd3d_hip.so
tmp=$(mktemp -d)
cp $cur $tmp/new.so && cp $parent $tmp/parent.so || exit 1
trap 'cp $tmp/new.so $cur; rm -rf $tmp' EXIT
legs=()
for r in $(seq $reps); do
  for n in parent new; do
    cp $tmp/$n.so $cur
    timeout -k 10 240 python experiments/attn_x3_tile_ab.py leg $table $n $tmp/leg_${r}_$n.json || { echo "leg $r $n failed: stopping"; exit 1; }
    legs+=($tmp/leg_${r}_$n.json)
  done
done
python experiments/attn_x3_tile_ab.py collect $out "${legs[@]}"
