#!/bin/bash
# Compiles the non-default settings of the switches that the ray kernels and k_shade still carry - the measurement builds and the alternative forms the tools
# drive - for gfx950 (device code only, nothing is linked or run), so that they do not rot unbuilt. Experiments that were measured negative are not here: they
# left the sources (docs/HISTORY.md, "Retired experiments"). Runs without a GPU: bash tools/check_variants.sh [jobs] > profiles/variants_compile.txt
# A variant is a set of -D flags; it is compiled into the fast flavour's two translation units (wavefront_fast.hip, wavefront_fast_shadow.hip), and - where the
# host side takes part (leaf size, diagnostic counters) - into the exact flavour's unit (wavefront_exact.hip), core.hip and scene_device.hip with the exact flags.
cd "$(dirname "$0")/.." || exit 1
JOBS=${1:-4}
HIPCC=${ROCM_PATH:-/opt/rocm}/bin/hipcc
COMMON="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Os -fno-slp-vectorize --cuda-device-only -c -o /dev/null"
FAST="-DLUM_FAST=1 -ffp-contract=fast -fno-hip-fp32-correctly-rounded-divide-sqrt -freciprocal-math -fno-math-errno -fapprox-func -fgpu-flush-denormals-to-zero"
EXACT="-ffp-contract=off -fno-fast-math"
VARIANTS=(
  "phase_stats:-DLUM_PHASE_STATS:core"
  "leaf4:-DLUM_LEAF_MAX=4:core"
  "root_reference_form:-DLUM_ROOT_THRESHOLD=0:"
  "root_threshold_no_key:-DLUM_ROOT_KEY=0:"
  "root_integer_selects:-DLUM_ROOT_KEY=2:"
  "ablate_all:-DLUM_ABLATE=7 -DLUM_ABLATE_LIGHT=7:"
)
one() {
  local name=${1%%:*} rest=${1#*:}
  local flags=${rest%%:*} extra=${rest#*:}
  local ok=1 log
  for unit in "luminary_amd/csrc/device/wavefront_fast.hip $FAST -DLUM_SHADOW_KERNEL_EXTERN=1" "luminary_amd/csrc/device/wavefront_fast_shadow.hip $FAST" \
              ${extra:+"luminary_amd/csrc/device/wavefront_exact.hip $EXACT -DLUM_SHADOW_KERNEL_EXTERN=1"} ${extra:+"luminary_amd/csrc/host/core.hip $EXACT"} ${extra:+"luminary_amd/csrc/host/scene_device.hip $EXACT"}; do
    # shellcheck disable=SC2086
    if ! log=$($HIPCC $COMMON $flags ${unit#* } ${unit%% *} 2>&1); then ok=0; echo "---- $name: ${unit%% *}"; echo "$log" | grep -E "error|Error" | head -5; fi
  done
  if [ $ok = 1 ]; then echo "[ok]     $name ($flags)"; else echo "[FAILED] $name ($flags)"; fi
}
export -f one; export HIPCC COMMON FAST EXACT
echo "# tools/check_variants.sh: non-default switch settings compiled for gfx950 (device code only), $(date -u +%Y-%m-%d), source $(git rev-parse --short HEAD 2>/dev/null)"
printf '%s\n' "${VARIANTS[@]}" | xargs -P "$JOBS" -I{} bash -c 'one "$@"' _ {}
