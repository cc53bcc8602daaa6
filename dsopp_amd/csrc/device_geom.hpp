// Device-side camera-model predicates shared by the BA sweeps and the aligner (templated on the evaluation scalar S).
#pragma once
#include <hip/hip_runtime.h>

namespace dsopp_hip {

template <typename S>
__host__ __device__ __forceinline__ bool insideROI(S u, S v, S width, S height) {
  // CameraModelBase::insideCameraROI — camera_model_base.hpp:52-60 (border 4)
  return (u >= S(4)) && (v >= S(4)) && (u <= width - S(5)) && (v <= height - S(5));
}
template <typename S>
__host__ __device__ __forceinline__ bool validIdepth(S idepth) {
  // CameraModelBase::validIdepth — camera_model_base.hpp:67-74
  return idepth > S(-1e-4) && idepth < S(1.0 / 0.001 + 1e1);
}

/** where the aligner samples the reference image for a caller's point (u, v): its own texel cell when the point lies inside the
 *  camera ROI, so that the cell's four texels (ix .. ix + 1, iy .. iy + 1) exist; otherwise — outside, or not a finite number, which
 *  fails every comparison — texel cell (0, 0) with zero offsets, and `false`: the sweep never uses such a point (reprojectPattern's
 *  reference ROI test, camera_reproject.hpp:278-280), so its intensity is left 0 instead of being read from outside the level */
template <typename S>
__host__ __device__ __forceinline__ bool referenceSampleSite(S u, S v, int width, int height, int &ix, int &iy, S &dx, S &dy) {
  const bool inside = insideROI(u, v, static_cast<S>(width), static_cast<S>(height));
  const S x = inside ? u : S(0), y = inside ? v : S(0);  // (selected before the conversion: int(huge) and int(NaN) are undefined)
  ix = static_cast<int>(x);
  iy = static_cast<int>(y);
  dx = x - static_cast<S>(ix);
  dy = y - static_cast<S>(iy);
  return inside;
}

/** a caller's explicit reference point the aligner accepts: finite and of a magnitude whose products with the reprojection matrices stay
 *  finite in float as well.  The sweep predicates an invalid point's weight to zero but still evaluates its Jacobian row, and 0 x (inf or
 *  NaN) would poison the sums, so such a point is refused at the interface instead (points merely outside the ROI are fine: they are
 *  finite and weigh nothing) */
__host__ __device__ inline bool referencePointFinite(double u, double v, double idepth) {
  const double kMax = 1e15;
  return (u >= -kMax && u <= kMax) && (v >= -kMax && v <= kMax) && (idepth >= -kMax && idepth <= kMax);  // NaN fails every comparison
}

}  // namespace dsopp_hip
