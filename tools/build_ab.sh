#!/bin/bash
# A/B library builds of the product sources with extra -D flags, into ab_libs/<name>.so
# (tools/ab.py, tools/ab_bench.sh, kbench via SLG_LIB).   bash tools/build_ab.sh <name> [-DFLAG=V ...]
# Sources and flags are build.py's.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
name=$1; shift
mkdir -p "$R/ab_libs"
python3 "$R/structured_light_for_3d_model_replication_amd/build.py" --out "$R/ab_libs/$name.so.tmp" "$@"
mv "$R/ab_libs/$name.so.tmp" "$R/ab_libs/$name.so"
echo "built ab_libs/$name.so $*"
