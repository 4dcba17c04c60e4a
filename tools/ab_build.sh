#!/bin/bash
# Builds variants of the HIP library for A/B runs on the GPU box:
#   [AB_TU=sd_train] tools/ab_build.sh name1 "-DFOO=1" name2 "-DFOO=2" ...
# -> soccerdiffusion_amd/lib/variants/lib_<name>.so   (run with SD_HIP_LIB=<path> python bench.py ...)
# Only the translation unit AB_TU (default sd_traj: the tuned step kernels) is recompiled, with the product's flags for that unit plus the
# variant's (soccerdiffusion_amd.build.build_variant); the other objects come from the regular build (python -m soccerdiffusion_amd.build),
# which must be current.
set -e
cd "$(dirname "$0")/.."
TU=${AB_TU:-sd_traj}
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  python -m soccerdiffusion_amd.build --variant "$TU" "$name" $flags &
done
wait
ls -la soccerdiffusion_amd/lib/variants/
