#!/bin/bash
# Builds the HIP library for gfx950 in-tree: dsopp_amd/lib/libdsopp_hip.so (+ libdsopp_hip_tools.so: counter-calibration kernels)
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
OUT="${DSOPP_HIP_OUT:-$HERE/../lib}"
mkdir -p "$OUT"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
# -amdgpu-kernarg-preload-count=16: the dispatcher hands the first 16 argument words to every wave in scalar registers (gfx940+), so a
# kernel whose first loads depend on its leading pointer arguments alone starts them in its first cycles instead of behind an
# argument fetch (the sweep, reduction and solve launches are laid out for this: profiles/r05/prologue_kernel_stats.txt)
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -Wall -Wno-unused-function -mllvm -amdgpu-kernarg-preload-count=16 ${DSOPP_HIP_EXTRA_FLAGS:-}"
# align.hip: the persistent tracker kernel's control step is ONE wave running a ~600-instruction dependency chain (8 x 8 LDL^T, SE3 exp): the
# default scheduler orders for register pressure and puts whole FMA chains in front of every pivot; max-ilp interleaves the independent
# updates with the reciprocal chains (profiles/r06/tracker_*: control step 1.76 -> see DESIGN.md section 4)
FLAGS_align="${DSOPP_HIP_ALIGN_SCHED--mllvm -amdgpu-sched-strategy=max-ilp}"
# optical_flow.hip: the tracker's float steps are single IEEE operations in a stated order (include/dsopp_hip.h): no product and sum may fuse
FLAGS_optical_flow="-ffp-contract=off"
# rotation_ransac.hip: the products and sums of the stated binary64 arithmetic stay unfused, as the NumPy model takes them
FLAGS_rotation_ransac="-ffp-contract=off"
# orb.hip: the Harris response is a chain of single IEEE binary32 steps in a stated order (include/dsopp_hip.h), as the NumPy model takes them
FLAGS_orb="-ffp-contract=off"
# geometric_ba.hip: the cost of a state is the same bits wherever a kernel evaluates it (the linearisation and the candidate pass share one residual)
FLAGS_geometric_ba="-ffp-contract=off"
# pnp_ransac.hip: the quartic's coefficients, the scores and the refinement's sums are single IEEE binary64 steps in the stated order, as the NumPy model takes them
FLAGS_pnp_ransac="-ffp-contract=off"
# two_view_ransac.hip: the cubics' coefficients, the scores and both refinements' sums are single IEEE binary64 steps in the stated order, as the NumPy model takes them
FLAGS_two_view_ransac="-ffp-contract=off"
# marginalization.hip: the frame scores are single IEEE binary64 steps in the stated order, as the NumPy model takes them
FLAGS_marginalization="-ffp-contract=off"
# debug_views.hip: the average, the state M and the levels are single IEEE binary64 steps in the stated order, as the NumPy model takes them
FLAGS_debug_views="-ffp-contract=off"
# point_cloud.hip: the positions of the exported cloud are single IEEE binary64 steps in the stated order, as the NumPy model takes them
FLAGS_point_cloud="-ffp-contract=off"
# camera_remap.hip: a map entry is a chain of single IEEE binary64 steps in the stated order (include/dsopp_hip.h), as the NumPy model takes them
FLAGS_camera_remap="-ffp-contract=off"
pids=()
for src in pyramid undistort camera_remap transform colour optical_flow rotation_ransac geometric_ba pnp_ransac two_view_ransac orb semantics marginalization debug_views point_cloud pba align depth_estimation features features_eigen comm calibration window_group; do
  if [ -f "$HERE/$src.hip" ]; then
    extra="FLAGS_$src"
    $HIPCC $FLAGS ${!extra:-} -c "$HERE/$src.hip" -o "$OUT/$src.o" &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait "$p"; done
objs=()
for src in pyramid undistort camera_remap transform colour optical_flow rotation_ransac geometric_ba pnp_ransac two_view_ransac orb semantics marginalization debug_views point_cloud pba align depth_estimation features features_eigen comm window_group; do [ -f "$OUT/$src.o" ] && objs+=("$OUT/$src.o"); done
$HIPCC --offload-arch=gfx950 -shared -fPIC "${objs[@]}" -o "$OUT/libdsopp_hip.so"
# measurement aids that are not part of the product (gather kernels of known geometry for the counter calibration, scripts/pmc_target.py)
[ -f "$OUT/calibration.o" ] && $HIPCC --offload-arch=gfx950 -shared -fPIC "$OUT/calibration.o" -o "$OUT/libdsopp_hip_tools.so"
echo "built $OUT/libdsopp_hip.so"
