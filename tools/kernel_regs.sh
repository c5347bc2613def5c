#!/bin/bash
# VGPR / SGPR / scratch of every device kernel of the library (each .hip translation unit of
# build.py's list, product flags plus any extra -D flags given):
#   bash tools/kernel_regs.sh [-DFLAG=V ...] [| grep main3]
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
python3 "$R/structured_light_for_3d_model_replication_amd/build.py" --device "$T" "$@" 2>/dev/null
for co in "$T"/*.co; do
  /opt/rocm/lib/llvm/bin/clang-offload-bundler --unbundle --type=o --input="$co" \
    --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output="$co.o"
  /opt/rocm/lib/llvm/bin/llvm-readelf --notes "$co.o" | grep -E "^ +\.name:|\.vgpr_count:|\.sgpr_count:|\.private_segment_fixed_size:" \
    | paste - - - - | awk '{print $2, "scratch="$4, "sgpr="$6, "vgpr="$8}'
done
rm -rf "$T"
