#!/bin/bash
# tools/build_variant.sh <name> "<extra hipcc flags>" [source dir]  ->  probes/variants/lib_<name>.so  (experiment builds for same-box A/B runs:
# tools/gpu_variants.py; git-ignored, shipped to the GPU box with the tree)
set -e
NAME=$1; FLAGS=$2; SRC=${3:-density_amd/csrc}
mkdir -p probes/variants
# the sources are density_amd/build.py's list (an older source dir has fewer of them)
SOURCES=$(cd "$(dirname "$0")/.." && python3 -c "from density_amd.build import SOURCES; print(' '.join(SOURCES))")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -w -DDENSITY_HIP_DEBUG -DDENSITY_HIP_KERNELS_ID="\"variant-$NAME\"" $FLAGS -o probes/variants/lib_$NAME.so \
  $(for f in $SOURCES; do [ -f $SRC/$f ] && echo $SRC/$f; done)
ls -la probes/variants/lib_$NAME.so
