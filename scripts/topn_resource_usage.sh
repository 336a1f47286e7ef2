#!/bin/bash
# usage: scripts/topn_resource_usage.sh [root of the tree to compile, default: this one] [out directory, default: <root>/profiles]
# The compiler's resource report (-Rpass-analysis=kernel-resource-usage) of the four batched top-N units whose tile kernels share
# tb_select.hpp, one device-only compile per unit and precision with the product build's flags:
#   <out>/topn/kernel_resource_usage.txt  <out>/topn_quota/kernel_resource_usage.txt  <out>/topn_shared/kernel_resource_usage.txt
#   <out>/topn_weighted/kernel_resource_usage.txt
# and of the diversified top-N and the deep unit whose chunk loop it calls:
#   <out>/topn_diverse/kernel_resource_usage.txt  <out>/topn_diverse/topn_deep_kernel_resource_usage.txt
# and of the top-N with per-(user, item) score factors (its dense tile kernel, its sparse kernel and its merge):
#   <out>/topn_adjusted/kernel_resource_usage.txt
set -e
ROOT=$(cd "${1:-$(dirname "$0")/..}" && pwd)
OUT=${2:-$ROOT/profiles}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -Wno-unused-function -Wno-unused-const-variable -Wno-pass-failed"
for unit in topn:topn_batch topn_quota:topn_quota topn_shared:topn_shared topn_weighted:topn_weighted topn_diverse:topn_diverse topn_diverse:topn_deep topn_adjusted:topn_adjust; do
  dir=${unit%%:*}; src=${unit##*:}
  file=kernel_resource_usage.txt
  [ "$src" = topn_deep ] && file=topn_deep_kernel_resource_usage.txt
  mkdir -p "$OUT/$dir"
  {
    echo "# hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage -c poismf_amd/csrc/$src.hip (the build's flags; scripts/topn_resource_usage.sh)"
    for flavour in "-DUSE_FLOAT" ""; do
      echo
      echo "## flavour: ${flavour:-double (no flag)}"
      ${HIPCC:-/opt/rocm/bin/hipcc} $FLAGS $flavour --cuda-device-only -c -Rpass-analysis=kernel-resource-usage -o /dev/null "$ROOT/poismf_amd/csrc/$src.hip" 2>&1 |
        sed -n 's/^.*remark: \(.*\) \[-Rpass-analysis=kernel-resource-usage\]$/\1/p'
    done
  } > "$OUT/$dir/$file"
done
