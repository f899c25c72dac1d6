#!/bin/bash
# build kernel variants: scripts/variants.sh name1:"-DX=0 -DY=1" name2:...   -> sage_amd/libsage_hip_<name>.so
# (knobs: the block of tuning constants at the head of sage_amd/csrc/kernels.hip — SAGE_PRELIM_WAVES, SAGE_RESCORE_WAVES, SAGE_NARROW_WAVES,
# SAGE_PROBE_PER_LANE, SAGE_PROBE_CELLS, SAGE_TILE8_CELLS, SAGE_MARK_BLOCKS8 / 16, SAGE_COOP_MIN_HITS, SAGE_COOP_MAX_LANES — and -DSAGE_HIP_EXPERIMENTS;
# A/B them on the GPU with scripts/ab_libs.sh)
for spec in "$@"; do
  name=${spec%%:*}; flags=${spec#*:}
  SAGE_HIP_LIB=$PWD/sage_amd/libsage_hip_$name.so SAGE_HIP_OBJ_SUFFIX=_$name SAGE_HIP_EXTRA_FLAGS="$flags" python -m sage_amd.build --force 2>&1 | grep -i "error" &
done
wait; ls -la sage_amd/libsage_hip_*.so
